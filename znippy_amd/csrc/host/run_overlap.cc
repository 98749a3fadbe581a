// The overlap rule of the run lanes: a pure function of two run descriptions.  `next` may execute beside
// `prev` only when neither can see the other: both are lean lane runs (one kernel that depends on nothing but its own
// cursor, no pool of the context), they use different sets of per-run device state, whatever both write is the same
// bytes or lands in different places, and neither reads where the other writes.
#include "run_overlap.h"

extern "C" int zn_regions_disjoint(uint64_t a, uint64_t a_len, uint64_t b, uint64_t b_len) {
    if (a_len == 0 || b_len == 0) return 1;
    if (a + a_len < a || b + b_len < b) return 0;  // wraps: where it ends is anybody's guess
    return a + a_len <= b || b + b_len <= a;
}

static bool same_arguments(const zn_run_desc &p, const zn_run_desc &n) {
    return p.table == n.table && p.d_blobs == n.d_blobs && p.blob_base == n.blob_base && p.blob_cap == n.blob_cap &&
           p.verify_only == n.verify_only && (p.verify_only || (p.d_out == n.d_out && p.out_cap == n.out_cap));
}

extern "C" int zn_runs_may_overlap(const zn_run_desc *prev, const zn_run_desc *next) {
    if (!prev || !next) return 0;
    const zn_run_desc &p = *prev, &n = *next;
    if (!p.lane_run || !n.lane_run) return 0;
    if (p.table == n.table && p.slot == n.slot) return 0;  // the same control block, digests and corrupt list
    // The same table read from the same blobs into the same place: by the contract of the async calls the blobs of a queued
    // run do not change before its results are read, so both runs write the same bytes (a pipeline over one buffer pair).
    if (same_arguments(p, n)) return 1;
    // From here on the regions decide.  A blob region of undeclared size cannot be compared with anything.
    const bool p_writes = !p.verify_only, n_writes = !n.verify_only;
    if (p_writes && n_writes && !zn_regions_disjoint(p.d_out, p.out_cap, n.d_out, n.out_cap)) return 0;  // two writers, one place
    if (n.blob_cap == ZN_BLOB_CAP_UNDECLARED) return 0;  // (only the identical case qualifies)
    if (p_writes && !zn_regions_disjoint(n.d_blobs, n.blob_cap, p.d_out, p.out_cap)) return 0;  // next reads where prev writes
    if (n_writes) {  // next writes where prev still reads
        if (p.blob_cap == ZN_BLOB_CAP_UNDECLARED) return 0;
        if (!zn_regions_disjoint(p.d_blobs, p.blob_cap, n.d_out, n.out_cap)) return 0;
    }
    return 1;
}
