// The plan of one write-side run (enc_plan.h).  The stages that carry it out are in api.hip (rounds_launch).
#include "enc_plan.h"

#include <algorithm>

int enc_window_log(const EncEnv &e) {
    return e.level >= ENC_HIGH_TIER_LEVEL ? e.window_log : 0;  // (the fast tier keeps its frames)
}

// one share of the items: the wide or the small variant's first launch
static EncLaunch enc_share(const EncShape &s, uint32_t n_items, int g) {
    EncLaunch l{};
    l.on = n_items != 0;
    if (!l.on) return l;
    l.n_items = n_items;
    l.use_order = !(n_items == s.n_items);  // all of one kind: no indirection
    l.batch = std::max<uint32_t>(1, std::min<uint32_t>(16, n_items / (uint32_t)(g * 2)));
    l.grid = std::min<int>(g, (int)n_items);
    return l;
}

EncPlan enc_plan(const EncShape &s, const EncEnv &e) {
    EncPlan p{};
    p.high = e.level >= ENC_HIGH_TIER_LEVEL;
    p.window_log = enc_window_log(e);
    p.tail_mark = p.high && !p.window_log;  // the empty closing block says every block stands alone: not with a window
    // (any failure of the far window's allocations leaves it off for the call — the near window still works)
    p.far = p.window_log && s.ldm_entries && e.ldm_ok;
    p.store_decide = s.store_incompressible;
    p.pad = s.blob_align > 1;
    p.emit_tree = s.emit_tree && !e.nohash;  // (the diagnostic no-hash switch leaves nothing to make entries from)
    p.tree_out = p.emit_tree && s.n_tree_entries;
    // Tables of small encoded rounds only: the encoder's waves hash the rounds they are about to encode (EncodeArgs::fuse_tiles)
    // (Block tree: fuse_tiles is only set for tables whose every round is one piece, at most one 128 KiB block — n_items == n,
    // rounds_hash_plan — and a round of at most one block has no entries: such a table's tree is empty, and the entry kernel,
    // which hash_rounds_async queues behind the merge of big units, has nothing to do on this route.)
    p.fuse_hash = s.fuse_tiles && !s.store_incompressible && !e.nohash && !e.no_fuse_hash;
    // checksum over the ORIGINAL bytes (stream_packer.rs:L219): VALU-bound, submitted to the
    // auxiliary stream right after the persistent (latency-bound) encoder so both share the CUs
    // Store-heavy table (most bytes are skip rounds): hashing and copying the stored bytes are one pass over them once
    // their blob offsets are known — scan and gather run first (the gather leaves the stored pieces alone), then the
    // hash kernel copies what it hashes.  Otherwise the hash runs beside the encoder on the auxiliary stream.
    // (Blobs are packed without gaps by default, so behind a compressed round the offsets are odd: unless every round is
    // stored and every length a multiple of 16 — or the table asks for blob offsets aligned to 16 bytes or more — the
    // launch uses the kernel variant that re-cuts the bytes to 16-byte boundaries on their way out: plain 16-byte stores
    // at odd addresses cost more than the pass they save.)
    const bool heavy = s.in_bytes && (s.in_bytes - s.enc_bytes) * 2 >= s.in_bytes;
    p.fuse_store = heavy && !s.store_incompressible &&
                   !e.no_fused_store && !e.nohash;
    p.fork_aux = !p.fuse_store && !p.fuse_hash;
    p.hash_beside = p.fork_aux && !e.nohash;
    // lane-per-piece gather (64 consecutive pieces per wave): only for tables without blocks above 16 KiB — the consecutive
    // blocks of one big round land in one wave, which then copies them one after the other (a table of 4,900 text files, a
    // few of them above 1 MiB: 0.29 ms against 0.03 for a wave per piece).  Store-heavy table: the stored rounds' 64 KiB
    // slices are not copied here (the hash kernel does it) — only their bookkeeping is left, a lane's work.
    p.small_pieces = s.n_items && s.n_wide == 0 && (p.fuse_store || s.in_bytes / s.n_items <= 16384);
    // the wide share first: its blocks are the long ones
    p.wide = enc_share(s, s.n_wide, e.encode_grid);
    p.small = enc_share(s, s.n_small, e.encode_grid_small);
    if (p.small.on && p.fuse_hash)  // the cursor counts tiles
        p.small.grid = std::min<int>(e.encode_grid_small, (int)((s.plan_n_tiles + s.fuse_tiles - 1) / s.fuse_tiles));
    if (s.n_small) {  // second wide launch: whatever the small variant handed over (count on the device)
        p.retry.on = true;
        p.retry.n_items = s.n_small; p.retry.use_order = true;  // (its list is the small variant's hand-over list)
        p.retry.batch = 1;
        p.retry.grid = std::min<int>(e.encode_grid, (int)s.n_small);
    }
    return p;
}
