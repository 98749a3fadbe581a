// The compiled host layer's read-side decisions (znippy_host.cpp): everything it works out from the index — untrusted input — before
// it reads a byte of the archive: which blobs are read and where they land in the pinned slab, what a private row table says a
// row's extent is, how a byte range of a file maps to chunks, which rows a rank, a batch and a writer thread take, whether a
// sidecar's layout agrees with the index.  Plain C++, no HIP call, no file descriptor: a stand-alone program checks all of it
// under the sanitizers on adversarial columns (tests/test_read_plan_cpu.py).  znippy_host.cpp does the I/O the plans describe.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "range_plan.h"  // tree_entries_of

namespace zn {

// the one status code the plans give out: ZNIPPY_E_CORRUPT of include/znippy_hip.h (znippy_host.cpp asserts that it is)
constexpr int32_t RDP_OK = 0, RDP_E_CORRUPT = -5;

// The eight base columns of the index (index.rs:L43-54), read-only.  Nothing here is trusted: offsets and sizes are any 64-bit value.
struct IndexView {
    const std::string *path = nullptr;
    const uint32_t *chunk_seq = nullptr;
    const uint64_t *fdata_offset = nullptr;
    const uint8_t *compressed = nullptr;  // one byte per row
    const uint64_t *usize = nullptr, *blob_offset = nullptr, *blob_size = nullptr;
    const uint8_t *checksum = nullptr;  // 32 bytes per row
    uint64_t n = 0, file_size = 0;
    // bytes of a row: uncompressed_size, or blob_size for a stored row — a stored row is its blob (decompress.rs:L160-166)
    uint64_t row_len(uint64_t r) const { return compressed[r] ? usize[r] : blob_size[r]; }
    bool blob_in_file(uint64_t r) const { return blob_offset[r] <= file_size && blob_size[r] <= file_size - blob_offset[r]; }
    uint64_t tree_entries(uint64_t r) const { return tree_entries_of(row_len(r)); }
    const uint8_t *ck(uint64_t r) const { return checksum + 32 * r; }
};

// The columns of a private znippy_rows_create, and per row where its blob bytes lie in the archive file.  add() packs the blobs
// back to back: row k's bytes belong at bo[k] = the sum of the blobs before it, in a slab of `sum` bytes.
struct SlabRead { uint64_t fpos, at, len; };  // len bytes at fpos of the archive file -> slab + at
struct RowTable {
    std::vector<uint64_t> bo, bs, us, fpos;
    std::vector<uint8_t> bitmap, ck;  // ck: 32 bytes per row, or empty (a table without checksums)
    uint64_t sum = 0;
    size_t n() const { return bo.size(); }
    bool comp(size_t k) const { return (bitmap[k >> 3] >> (k & 7)) & 1; }
    size_t add(uint64_t file_pos, uint64_t blob_size, uint64_t len, bool compressed, const uint8_t *checksum32);
    // rows `list` of this table as a table of their own over the SAME slab: bo and sum are this table's
    RowTable subset(const std::vector<size_t> &list) const;
    std::vector<SlabRead> reads() const;  // one per row with a blob: fpos[k] -> bo[k]
};

// ---- whole rows (decode_range) ----
struct RowsRead {
    int32_t rc = RDP_OK;
    const char *err = nullptr;
    RowTable t;                     // bo: relative to `base`
    std::vector<uint64_t> out_off;  // position of each row's bytes in the decoded region (its length is t.us)
    uint64_t total = 0;             // bytes of the decoded region
    uint64_t base = 0, nblob = 0;   // the slab holds archive bytes [base, base + nblob) (span), or the packed blobs (base = 0)
    std::vector<SlabRead> reads;
};
RowsRead plan_rows_read(const IndexView &v, const uint64_t *row_ids, size_t n, bool verify);

// ---- byte ranges of files ----
// The chunks of one file that bytes [off, off + len) touch (off + len saturates at 2^64 - 1).  rows: the file's rows sorted by
// fdata_offset.  Per touched chunk: the archive row, the first byte wanted inside it and how many.  *covered: the bytes found —
// less than len where the range reaches past the end of the file or over a hole between chunks.  RDP_E_CORRUPT at the first
// touched chunk whose blob is not inside the archive file.
struct RangeHit { uint64_t row, begin, len; };
int32_t map_range(const IndexView &v, const uint64_t *rows, size_t n_rows, uint64_t off, uint64_t len, std::vector<RangeHit> *hits, uint64_t *covered);

struct RangeList {  // the range columns of znippy_rows_read_ranges: table row, first byte, length
    std::vector<uint64_t> row, begin, len;
    size_t n() const { return row.size(); }
    void add(uint64_t r, uint64_t b, uint64_t l) { row.push_back(r); begin.push_back(b); len.push_back(l); }
};
// znippy_archive_read_range[_verified]: whole blobs of the touched chunks, clipped at the end of the file — a short read, as pread
struct RangeRead {
    int32_t rc = RDP_OK;
    RowTable t;                  // with checksums if verify
    RangeList rg;                // range k is of table row k
    std::vector<uint64_t> arow;  // table row -> archive row
    uint64_t total = 0;
};
RangeRead plan_range_read(const IndexView &v, const uint64_t *rows, size_t n_rows, uint64_t off, uint64_t len, bool verify);

// One pass of znippy_archive_extract_zip_entries: many requests, each wholly inside its file or ZNIPPY_E_CORRUPT (the index does
// not cover the file).  Of a stored chunk only the requested bytes are read and uploaded, as a stored row of their own (a jar is
// stored by the extension rule, and of a jar of many MB the three passes want the tail, the directory and one entry); of a
// compressed chunk the whole frame, once per pass however many requests touch it.
struct FileRange {
    const std::vector<uint64_t> *rows;  // the file's archive rows, sorted by fdata_offset
    uint64_t off, len;
};
struct FileRangesRead {
    RowTable t;
    RangeList rg;
    std::vector<size_t> of_req;  // range -> request
    std::vector<uint64_t> at;    // request -> where its bytes start in the gathered output
    std::vector<int32_t> st;     // request -> 0 or RDP_E_CORRUPT
    uint64_t total = 0;
};
FileRangesRead plan_file_ranges(const IndexView &v, const std::vector<FileRange> &req);

// ---- decompress_archive: ranks, batches, writers ----
// Contiguous [begin,end) per rank, balanced by sum(weights); rank < world
std::pair<uint64_t, uint64_t> split_rows(const uint64_t *w, uint64_t n, uint32_t rank, uint32_t world);

// Unique paths (decompress.rs:L64-69) and the first row of every path: where its file is created.  Rows of a path that are not
// adjacent (duplicate entries) clear `adjacent`: they force a single writer so that the first-touch truncate cannot race with a
// later row's write.  per_rank (several ranks write into the same files): first touch is the first row of a path inside
// [begin, end), and comes with the file's final length.  Ranks write disjoint parts of a file in any order, so none of them may
// O_TRUNC; instead every rank sets the file to its final length when it first touches it (idempotent: every row lies inside that
// length) — a longer file left from an earlier run loses its stale tail.
struct FirstTouch {
    std::vector<uint8_t> first;  // per row
    bool adjacent = true;
    size_t n_unique = 0;
    std::unordered_map<std::string, uint64_t> final_size;  // per_rank only
};
FirstTouch read_plan_first_touch(const IndexView &v, uint64_t begin, uint64_t end, bool per_rank);

// Rows [i, j) of one decoded batch: as many as cost no more than batch_bytes, and at least one.  A row costs its decoded bytes;
// under verify_only — nothing is written, so what a batch takes on the device is its blobs and the scratch of its compressed rows —
// its blob and, if compressed, its decoded bytes.  Returns j <= end.
uint64_t cut_batch(const IndexView &v, uint64_t i, uint64_t end, uint64_t batch_bytes, bool verify_only);

// Rows [0, n) of a decoded batch (archive rows i ..) among up to n_writers threads: contiguous parts [k0, k1) of about equal bytes,
// cut only where the path changes (a writer keeps one descriptor open).  Writers that CREATE files in one directory contend on its
// lock and are fastest at ~4 (tmpfs, 100k files: 1 writer 0.50 s, 2: 0.41 s, 4: 0.38 s, 8: 0.52 s, 16: 0.78 s, 32: 1.2 s).
std::vector<std::pair<uint64_t, uint64_t>> cut_writers(const uint64_t *out_off, uint64_t total, const std::string *paths, uint64_t i, uint64_t n, unsigned n_writers);

// ---- the block-tree sidecar `<archive>.b3t` ----
constexpr char B3T_MAGIC[9] = "ZNPYB3T1";
constexpr uint32_t B3T_BLOCK_LOG = 17;
constexpr size_t B3T_HEADER = 32;
// A sidecar of `size` bytes is usable if it is a header and whole 32-byte entries, the header names this format, this index's row
// count and the file's entry count, and the entries every row has by the index add up to that count.  first: n + 1 prefix sums.
bool sidecar_layout(const uint8_t *raw, uint64_t size, const IndexView &v, std::vector<uint64_t> *first);
// Appends the `entries` 32-byte entries at byte `at` of a packed tree buffer to *dst; returns the byte behind them.
size_t take_tree(const uint8_t *packed, size_t at, uint64_t entries, std::vector<uint8_t> *dst);

}  // namespace zn
