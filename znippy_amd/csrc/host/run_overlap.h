// May two read runs of a context execute side by side?  The description of a queued run and the rule (run_overlap.cc):
// plain C++, no HIP call, decided on the host when the second run is queued (api.hip: lane_begin).
#pragma once
#include <stdint.h>

#define ZN_BLOB_CAP_UNDECLARED (~0ull)

struct zn_run_desc {
    const void *table;     // the row table the run belongs to
    uint32_t slot;         // which of the table's two sets of per-run device state it uses
    uint8_t lane_run;      // a lean run on a run lane: one role-split kernel between the clear and the verify, no context pool
    uint8_t verify_only;   // writes no output (d_out / out_cap are not looked at)
    uint64_t d_blobs, blob_base, blob_cap;  // device address of the blob region; blob_cap = ZN_BLOB_CAP_UNDECLARED: size not known
    uint64_t d_out, out_cap;                // device address and size of the output region
};

extern "C" {
// 1: [a, a + a_len) and [b, b + b_len) share no byte.  An empty region shares none with anything; a region that wraps 2^64
// is not known to be disjoint from any non-empty one.
int zn_regions_disjoint(uint64_t a, uint64_t a_len, uint64_t b, uint64_t b_len);
// 1: `next` may be queued without an order behind `prev`, the run queued directly in front of it; 0: it waits for prev's kernel.
int zn_runs_may_overlap(const zn_run_desc *prev, const zn_run_desc *next);
}
