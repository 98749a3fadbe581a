// The host planning of znippy_tar_list_batch: which items pass, the lists and the scratch the kernels of tar_list.hip work on, how
// many rounds the chain stage runs, and the way from what the device reports to what the caller gets.
// Plain C++: no HIP call and no I/O, device addresses are only added to.  The totals and the member records come from device memory
// that was written while walking untrusted input, so nothing here trusts them: the totals of an item are checked against its size
// before they take room, and every member record is checked against its item (inside it, in stream order, names and contents
// packed without gap) before it becomes a gather piece or reaches the caller; a contradiction ends in a status for the item
// (tests/test_tar_list_cpu.py runs all of it under the sanitizers).
//
// Nodes.  An item of len bytes has len / 512 whole blocks and one end node behind them (the header boundary where its bytes end, or
// the header that is cut short).  The nodes of all items lie back to back; a chunk is up to TL_CHUNK nodes of one item, the work of one
// workgroup of the scan and emit launches.  Every per-node list is dense: there is no overflow path.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "range_plan.h"  // RangePiece, range_cut_pieces
#include "tar_list.h"    // znippy_tar_member

namespace zn {

// ---- what the kernels read and write (tar_list.hip) ----
constexpr uint32_t TL_CHUNK = 256;
struct TlItem {
    const uint8_t *base;  // the tar, any alignment
    uint32_t len, blocks; // blocks: whole ones; the end node is node `blocks`
    uint32_t first_node, first_chunk;
};
struct TlChunk { uint32_t item, first, n, pad; };  // nodes [first, first + n) of the item
struct TlNode {
    uint32_t succ;  // the node the header leads to (over all items); a terminal leads to itself
    uint32_t kind;  // tr::K_* | typeflag << 8
    uint64_t size;  // the size field
};
struct TlSum { uint64_t cnt, names, out; };  // of a chunk; after the prefix launch, of all chunks in front of it
struct TlTotal {
    uint64_t key;   // ~0: nothing failed; else node << 8 | TL_KEY_*: the first node on the chain, in stream order, that fails
    uint64_t cnt, names, out;  // the matching members of the chain, their names' bytes, their sizes
};
constexpr uint64_t TL_KEY_NONE = ~0ull, TL_KEY_CORRUPT = 1, TL_KEY_UNSUP = 2;
struct TlBase {  // where the members of an item go in the call's staging lists
    uint64_t member, names, out;
    uint32_t take, pad;
};

constexpr int32_t TL_OK = 0, TL_E_INVAL = -1, TL_E_NOMEM = -3, TL_E_DST_SMALL = -4, TL_E_CORRUPT = -5, TL_E_UNSUPPORTED = -6;
constexpr uint64_t TL_NODES_MAX = 1ull << 31;   // (succ and the node of a key are 32 bits)
constexpr uint64_t TL_FILTER_MAX = 1ull << 16;

struct TlCall {  // a view of the caller's arguments (n > 0; the NULL checks are api.hip's)
    const uint8_t *d_tar;
    uint64_t tar_cap;
    const uint64_t *tar_off, *tar_len;
    uint64_t n;
    znippy_tar_member *members;  // NULL with members_cap 0: measure mode
    uint64_t members_cap;
    char *names;
    uint64_t names_cap;
    uint8_t *d_out;  // NULL: no contents
    uint64_t out_cap;
    uint64_t *member_first;  // n + 1
    uint64_t *names_bytes, *out_bytes;
};
struct TlLayout {  // the one device allocation
    size_t items, chunks, filter, nodes, mark, jump_a, jump_b, pred, pick, src, sums, totals, bases, bytes;
};
struct TlBatch {
    bool measure = false;
    std::vector<int32_t> st;        // per array item
    std::vector<TlItem> items;      // [k]: the items that passed and have bytes
    std::vector<uint32_t> item_of;  // k -> array item
    std::vector<TlChunk> chunks;
    uint64_t n_nodes = 0;
    uint32_t max_nodes = 0;         // of one item
    std::vector<TlTotal> totals;    // [k], the device's (sized by tl_admit, filled by api.hip)
    std::vector<TlBase> bases;      // [k]
    uint64_t take_members = 0, take_names = 0, take_out = 0;  // what the taken items need of the staging lists
    std::vector<RangePiece> pieces;
};

// Every item: inside tar_cap or TL_E_INVAL (also where off + len wraps); 4 GiB or more is TL_E_UNSUPPORTED; no bytes is status 0
// with no list entry.  TL_OK or TL_E_NOMEM (the nodes above TL_NODES_MAX).  member_first, names_bytes and out_bytes are zeroed.
int tl_admit(const TlCall &c, TlBatch &b);
TlLayout tl_layout(const TlBatch &b, uint64_t filter_bytes);
// Rounds of pointer doubling that close a chain of max_nodes nodes: the smallest r with 2^r >= max_nodes
uint32_t tl_rounds(uint32_t max_nodes);
// Staging entries the call can need: members and name bytes (0 in measure mode), and the pieces of the gather.  TL_OK or TL_E_NOMEM.
int tl_staging(const TlCall &c, const TlBatch &b, size_t *members, size_t *names, size_t *pieces);
// The totals to statuses and room: an item whose totals contradict its size is TL_E_CORRUPT; one that no longer fits a cap is
// TL_E_DST_SMALL and takes no room.  Measure mode: member_first, names_bytes and out_bytes are final after this.
void tl_place(const TlCall &c, TlBatch &b);
// The member records and names of the taken items (staging lists, as the device wrote them by b.bases) into the caller's lists,
// checked record by record; an item with a record that contradicts it is TL_E_CORRUPT and takes no room.  The gather's pieces.
void tl_accept(const TlCall &c, TlBatch &b, const znippy_tar_member *recs, size_t n_recs, const char *names, size_t n_names);

}  // namespace zn
