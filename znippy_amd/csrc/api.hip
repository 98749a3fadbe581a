// C ABI of libznippy_hip.so (include/znippy_hip.h).  Host-side plumbing only: uploads of the
// index columns / Round tables, the tile plan that drives the kernels' work cursor, kernel
// launches on the context's HIP stream, and result read-back.
#include <unistd.h>
#include "common.h"
#include "encode.h"
#include "../../include/znippy_hip.h"
#include "host/enc_plan.h"
#include "host/gz_plan.h"
#include "host/range_plan.h"
#include "host/rows_plan.h"
#include "host/run_overlap.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <memory>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>
#include <unordered_map>

namespace zn {
int measure_b3_pass_ns(int cus, hipStream_t s, float *ns_per_pass_per_simd, float *ghz);
size_t decode_lit_scratch_bytes(int grid);
void set_fused_dbg(unsigned long long *p);
void set_fused_abl(int v);
}  // namespace zn

using namespace zn;
extern "C" void zn_rounds_totals(const uint64_t *len, const uint8_t *skip, size_t n, uint64_t out[8]);  // host/extents.cpp
extern "C" void zn_rows_extents(const uint64_t *bo, const uint64_t *bs, const uint64_t *oo, const uint64_t *us, size_t n, uint64_t out[8]);  // host/extents.cpp
extern "C" int zn_rows_pack32(const uint64_t *bo, const uint64_t *bs, const uint64_t *oo, const uint64_t *us, size_t n, uint32_t *dst);

#define HIPCHK(ctx, call)                                                                         \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                       \
            return ZNIPPY_E_HIP;                                                                  \
        }                                                                                         \
    } while (0)
// The body of an entry point whose work allocates host vectors sized by caller data: an allocation failure is an error code at the
// C boundary, not an exception through it.
#define ZN_NO_THROW(call) \
    try { return (call); } catch (const std::bad_alloc &) { return ZNIPPY_E_NOMEM; } catch (const std::length_error &) { return ZNIPPY_E_NOMEM; }
static_assert(RP_OK == ZNIPPY_OK && RP_E_INVAL == ZNIPPY_E_INVAL && RP_E_NOMEM == ZNIPPY_E_NOMEM && RP_E_DST_SMALL == ZNIPPY_E_DST_SMALL &&
              RP_E_CORRUPT == ZNIPPY_E_CORRUPT && RP_E_DIGEST == ZNIPPY_E_DIGEST, "host/range_plan.h gives out the codes of znippy_hip.h");
static_assert(RowsSwitches{}.bx_big == BX_BIG_SEQ, "host/rows_plan.h: the default of ZNIPPY_BX_BIG");

// diagnostic (ZNIPPY_TDBG): wall time of the sections of a table constructor
struct TDbg {
    bool on;
    const char *what;
    std::chrono::steady_clock::time_point t;
    std::string line;
    TDbg(bool on_, const char *what_) : on(on_), what(what_), t(std::chrono::steady_clock::now()) {}
    void mark(const char *name) {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        char b[96];
        snprintf(b, sizeof b, " %s=%.3f", name, std::chrono::duration<double, std::milli>(now - t).count());
        line += b;
        t = now;
    }
    ~TDbg() { if (on) fprintf(stderr, "[znippy tdbg] %s:%s ms\n", what, line.c_str()); }
};

struct KTime {
    const char *name;
    hipEvent_t t0, t1;
};

struct znippy_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string err;
    // decode scratch
    int decode_grid = 0;
    uint8_t *lit_scratch = nullptr;
    uint32_t *cursor = nullptr;
    // shim scratch (grow-only)
    uint8_t *shim_in = nullptr, *shim_out = nullptr;
    size_t shim_in_cap = 0, shim_out_cap = 0;
    // encoder scratch (grow-only) + tables
    int encode_grid = 0, encode_grid_small = 0;
    int gen_share = 3;  // workgroups per CU the general decoder takes while block items / foreign frames run beside it (4 = the whole register file)
    int level = 19;  // CompressCtx::new(compression_level), codec.rs:L16-28; CONFIG.compression_level is 19 (common_config.rs:L37)
    int window_log = 0;  // cross-block window of the higher effort tier (znippy_ctx_set_window_log); 0 = self-contained blocks
    uint64_t gz_cut = 0;  // znippy_ctx_set_gunzip_cut: the window of the block-start search of znippy_gunzip_batch in source bytes; 0 = no search
    uint64_t gz_cut_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // znippy_ctx_gunzip_cut_stats: the last gunzip call
    int batch_checksums = 0;  // the batch path takes frames with a content checksum and checks it itself (znippy_ctx_set_batch_checksums); read at the start of every run
    uint32_t *ldm = nullptr;  // far window index (grow-only, entries)
    size_t ldm_cap = 0;
    uint8_t *enc_prov = nullptr;
    size_t enc_prov_cap = 0;
    uint32_t *enc_seq = nullptr;
    EncTables *enc_tabs = nullptr;
    // auxiliary stream: the write side hashes on it while the main stream encodes
    hipStream_t aux = nullptr;
    hipStream_t copy = nullptr;  // result read-back of the write side (D2H beside the next run's kernels)
    uint8_t *lit_scratch_b = nullptr;  // literal scratch of the block-item launch (runs next to the general decoder)
    // pools of the two-phase path for foreign frames: decoded literals and 8-byte sequence records of every block of
    // every candidate frame of a run (grow-only, sized by the largest table seen; see ensure_fz_pools)
    uint8_t *fz_lit_pool = nullptr;
    unsigned long long *fz_seq_pool = nullptr;
    uint64_t fz_lit_cap = 0, fz_seq_cap = 0;
    // the batch path's table pools (zstd_batch.hip, k_bx_*): FSE decoding tables as 4-byte cells (the predefined ones at
    // the head), Huffman decoding tables as 2-byte cells
    uint16_t *bx_fse_pool = nullptr;
    uint16_t *bx_huf_pool = nullptr;
    uint64_t bx_fse_cap = 0, bx_huf_cap = 0;
    // the resolve path's word pool (k_rx_*: one 32-bit word per output byte of the big frames) and its chunk -> frame table
    uint32_t *rx_pool = nullptr, *rx_chunk = nullptr;
    uint8_t *rx_cdone = nullptr;
    uint64_t rx_cap = 0;  // words
    // verify-only runs (znippy_verify_rows): the region the rows that need bytes in memory are decoded into instead of a caller's
    // output (grow-only, ensure_verify_scratch); shared by every table and run of the context — runs are ordered on its stream
    uint8_t *vs_pool = nullptr;
    uint64_t vs_cap = 0;
    // range reads (znippy_rows_read_ranges): where the blocks and rows a call decodes land before their ranges are gathered (grow-only,
    // ensure_range_scratch).  [0] the blocks and the rows known up front to need a whole decode, [1] the rows a block pass gave up on
    uint8_t *rr_pool[2] = {nullptr, nullptr};
    uint64_t rr_cap[2] = {0, 0};
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_join2 = nullptr;
    // kernel timing
    std::vector<KTime> ktimes;
    int n_ktimes = 0;
    std::vector<hipEvent_t> event_pool;  // disable-timing events handed back by destroyed tables
    bool ktime_open = false;
    // page-locked host buffers handed back by destroyed tables: locking pages costs ~1 ms per 4 MB, more than a
    // whole C2 encode pass, so a table takes its result mirror from here when one is big enough
    std::vector<std::pair<size_t, void *>> pinned_pool;
    size_t pinned_pool_bytes = 0;
    std::vector<std::pair<size_t, void *>> dev_pool;  // device buffers handed back by destroyed tables
    std::unordered_map<void *, size_t> dev_sizes;     // capacity of every pooled-kind buffer that is in use
    size_t dev_pool_bytes = 0;
    // diagnostic switches (ZNIPPY_* environment), read ONCE when the context is created: nothing on the hot path
    // calls getenv
    struct : RowsSwitches {  // (the ones the read side's plan goes by: host/rows_plan.h)
        unsigned lds_pad = 0;    // ZNIPPY_LDS_PAD
        int store_g = 0;         // ZNIPPY_STORE_G: tiles per wave of the store path kernel (0 = from the tile count)
        bool edbg = false, no_fused_store = false, no_fork_verify = false, no_run_lanes = false, nohash = false, fz_only = false, tdbg = false, no_fuse_hash = false, trace = false, no_pack = false;
        int ktime = 2;  // per-kernel HIP events: 2 = every kernel, 1 = the dominant read kernels only, 0 = none
        bool poison = false;  // ZNIPPY_POISON (test hook): recycled and pooled memory is filled with poison_byte before it is handed out
        int poison_byte = 0;
    } sw;
    int poison_hold = 0;  // ZNIPPY_POISON: > 0 inside an entry point that has refilled the pools itself (poison_enter, PoisonHold)
    int cus = 256;
    // A lean run's verify is queued on the auxiliary stream, beside the next run's role-split kernel (run_verify): decided at
    // creation from what the two kernels take of a CU — a verify that cannot be resident beside that persistent kernel would
    // wait a whole step and stall the caller's lagged read
    bool fork_verify = false;
    // Run lanes: the main chain of a lean run — the wait for its slot, the clear, the role-split kernel, the
    // ev_main record — is queued on one of two run streams, run k of a table on lane k & 1.  Lane 0 is the context's main
    // stream, lane 1 a stream of its own (`lane`), so a read step stays within main + auxiliary + one more stream.  Two
    // consecutive lane runs that cannot see each other (zn_runs_may_overlap) are left unordered: the next run's clear executes
    // beside the previous run's kernel and its workgroups take each CU the moment the previous run's workgroup leaves it.
    // Only a context that owns its stream and forks its verify has lanes (lanes_on).
    //  - lane_join: the ev_main of the last run on `lane` that the main stream has not waited for yet.  Everything else a
    //    context queues goes to the main stream through ctx_enter (or rows_launch), which waits for it first (lanes_close).
    //  - main_dirty: work other than lane runs has been queued on the main stream since a lane run last ordered itself behind
    //    it.  The next lane run records ev_mark there; a run on `lane` waits for it (mark_pending: a run on lane 0 recorded
    //    it in front of itself and the next run on `lane` still has to wait).  Clear in a steady pipeline: nothing waits.
    //  - lane_prev: the lane run queued last (the predecessor: the one run the rule is asked about).  lane_hist[s]: the two runs
    //    queued last on stream s ([0] the later).  A lane run waits for the latest run on the OTHER stream that is older than its
    //    predecessor (everything older on that stream ended before it; everything older on its own stream ends before the run
    //    starts), so when a lane run starts nothing but its predecessor can still be executing: every pair of runs that can
    //    execute at the same time has been through the rule.
    //  - lane_ev[s]: the context's own events for that, two per stream taken in turn and recorded behind a run's ev_main (a
    //    table's ev_main is recorded again by the slot's next run: a wait for an older run would become a wait for a newer one).
    hipStream_t lane = nullptr;
    hipEvent_t ev_mark = nullptr, lane_join = nullptr;
    hipEvent_t lane_ev[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
    unsigned lane_n[2] = {0, 0};  // lane runs queued on each stream so far
    bool lanes_on = false, main_dirty = true, mark_pending = false;
    struct LaneRun { zn_run_desc d; hipEvent_t ev; bool on_lane, valid; } lane_prev = {}, lane_hist[2][2] = {};
    // znippy_ctx_run_lane_stats; [4]: lane runs that waited for a run OLDER than their predecessor that had not ended (znippy_ctx_run_lane_older_waits)
    uint64_t lane_stats[5] = {0, 0, 0, 0, 0};
    // Lifetime (znippy_hip.h): tables hold a reference to their context.  znippy_ctx_destroy with tables still alive only
    // closes the context (every call on it fails with ZNIPPY_E_INVAL from then on); its memory and device resources go
    // when the last table is destroyed.
    int live_tables = 0;
    bool closing = false;
    unsigned long long *clk_buf = nullptr;  // diagnostic (ZNIPPY_DBG & 32768): shader cycles / 100 MHz ticks of one wave
    // diagnostic (ZNIPPY_DBG & 8, ZNIPPY_DDBG, ZNIPPY_EDBG): phase stamps of the previous launch of a kernel, one buffer per
    // kind, allocated at first use on this context's device (diag_cycle)
    enum Diag { DIAG_FUSED, DIAG_ITEMS, DIAG_FZ, DIAG_GENERAL, DIAG_BX, DIAG_ENCODE, DIAG_N };
    unsigned long long *diag[DIAG_N] = {};
};

static void read_switches(znippy_ctx *ctx) {
    auto on = [](const char *n) { const char *v = getenv(n); return v && *v && *v != '0'; };
    if (const char *e = getenv("ZNIPPY_DBG")) ctx->sw.dbg = atoi(e);
    if (const char *e = getenv("ZNIPPY_LDS_PAD")) ctx->sw.lds_pad = (unsigned)atoi(e);
    ctx->sw.no_block_items = on("ZNIPPY_NO_BLOCK_ITEMS");
    ctx->sw.no_fused_blocks = on("ZNIPPY_NO_FUSED_BLOCKS");
    ctx->sw.ddbg = on("ZNIPPY_DDBG");
    ctx->sw.edbg = on("ZNIPPY_EDBG");
    ctx->sw.no_fused_store = on("ZNIPPY_NO_FUSED_STORE");
    ctx->sw.nohash = on("ZNIPPY_NOHASH");
    ctx->sw.no_roles = on("ZNIPPY_NO_ROLES");
    ctx->sw.no_fz = on("ZNIPPY_NO_FZ");
    ctx->sw.tdbg = on("ZNIPPY_TDBG");
    ctx->sw.trace = on("ZNIPPY_TRACE");
    ctx->sw.no_lean = on("ZNIPPY_NO_LEAN");  // A/B: every run launches the kernels behind the role-split one
    ctx->sw.no_fork_verify = on("ZNIPPY_NO_FORK_VERIFY");  // A/B, tests: every run's verify on the main stream, in front of the next run
    ctx->sw.no_run_lanes = on("ZNIPPY_NO_RUN_LANES");  // A/B, tests: every lean run's main chain on the main stream, in queue order
    ctx->sw.no_pack = on("ZNIPPY_NO_PACK");  // A/B: the index columns always as four 64-bit copies
    if (const char *e = getenv("ZNIPPY_STORE_G")) ctx->sw.store_g = atoi(e) == 1 ? 1 : (atoi(e) == 2 ? 2 : 0);  // A/B, tests: tiles per wave of the store path kernel
    ctx->sw.no_stored_only = on("ZNIPPY_NO_STORED_ONLY");  // A/B: tables without a compressed row through the fused small-row kernels (until round 3's last day)
    ctx->sw.no_rx = on("ZNIPPY_NO_RX");  // A/B: big foreign frames executed by a wave each (round 3's first form)
    ctx->sw.no_fuse_hash = on("ZNIPPY_NO_FUSE_HASH");  // A/B: the write side's hash as a kernel of its own beside the encoder (round 2)
    ctx->sw.no_bx = on("ZNIPPY_NO_BX");
    if (const char *e = getenv("ZNIPPY_BX_BIG")) { ctx->sw.bx_big = (unsigned)atoi(e); ctx->sw.bx_big_set = true; }  // A/B: foreign frames through the round-2 paths (serial decoder + wave-per-block two-phase path)
    if (const char *lv = getenv("ZNIPPY_LEVEL")) { const int v = atoi(lv); if (v >= 1 && v <= 22) ctx->level = v; }  // initial level of every context (tests, A/B runs)
    if (const char *wl = getenv("ZNIPPY_WINDOW_LOG")) { const int v = atoi(wl); if (v == 0 || (v >= WINDOW_LOG_MIN && v <= WINDOW_LOG_MAX)) ctx->window_log = v; }  // initial window of every context (host layer, tools)
    if (const char *gc = getenv("ZNIPPY_GZ_CUT")) {  // initial value of every context (host layer, tools)
        char *end = nullptr;
        const unsigned long long v = strtoull(gc, &end, 10);
        if (*gc >= '0' && *gc <= '9' && end && !*end && gzcut::cut_valid(v)) ctx->gz_cut = v;
    }
    if (const char *bc = getenv("ZNIPPY_BX_CHECKSUM")) { const int v = atoi(bc); if (v == 0 || v == 1) ctx->batch_checksums = v; }  // initial switch of every context (host layer, tools)
    if (const char *gs = getenv("ZNIPPY_GEN_SHARE")) { const int v = atoi(gs); if (v >= 1 && v <= 4) ctx->gen_share = v; }  // A/B
    ctx->sw.fz_only = on("ZNIPPY_FZ_ONLY");  // test hook: no serial fallback behind the two-phase path (what it leaves shows up as corrupt rows)
    if (const char *e = getenv("ZNIPPY_ROLES_MIN")) ctx->sw.roles_min = (unsigned)atoi(e);
    if (const char *e = getenv("ZNIPPY_KTIME")) ctx->sw.ktime = atoi(e);
    if (const char *e = getenv("ZNIPPY_POISON")) {  // test hook: a fill byte, 0 .. 255 (decimal or 0x..; zero is a fill byte like any other), unset = off
        char *end = nullptr;
        const long v = strtol(e, &end, e[0] == '0' && (e[1] == 'x' || e[1] == 'X') ? 16 : 10);
        if (*e && end && !*end && v >= 0 && v <= 255) { ctx->sw.poison = true; ctx->sw.poison_byte = (int)v; }
    }
}

// ---- ZNIPPY_POISON (test hook) ---------------------------------------------------------------------------
// With the switch on, no buffer reaches its user holding what its last user — or nobody — left in it: every buffer of the
// recyclers below and every pool of the context is filled with the switch's byte first.  A result that changes with the byte,
// or differs from a context without the switch, read something before anything wrote it.  Off: one bool tested per site.
// The fill of a device buffer is queued on the main stream — everything that used the buffer before is ordered there by the
// time it comes back to a recycler — and waited for: uploads into it are plain hipMemcpy, which nothing orders behind a stream.
static hipError_t poison_dev(znippy_ctx *ctx, void *p, size_t bytes) {
    if (!p || !bytes) return hipSuccess;
    const hipError_t e = hipMemsetAsync(p, ctx->sw.poison_byte, bytes, ctx->stream);
    return e != hipSuccess ? e : hipStreamSynchronize(ctx->stream);
}

static void *pinned_take(znippy_ctx *ctx, size_t bytes, size_t *cap) {
    size_t best = ctx->pinned_pool.size();
    for (size_t i = 0; i < ctx->pinned_pool.size(); i++)
        if (ctx->pinned_pool[i].first >= bytes && ctx->pinned_pool[i].first <= 4 * bytes + 4096 &&
            (best == ctx->pinned_pool.size() || ctx->pinned_pool[i].first < ctx->pinned_pool[best].first))
            best = i;
    if (best != ctx->pinned_pool.size()) {
        void *p = ctx->pinned_pool[best].second;
        *cap = ctx->pinned_pool[best].first;
        ctx->pinned_pool_bytes -= *cap;
        ctx->pinned_pool.erase(ctx->pinned_pool.begin() + best);
        if (ctx->sw.poison) memset(p, ctx->sw.poison_byte, *cap);  // (given back only once nothing queued still writes it: pinned_give's callers)
        return p;
    }
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes) != hipSuccess) return nullptr;
    *cap = bytes;
    if (ctx->sw.poison) memset(p, ctx->sw.poison_byte, *cap);
    return p;
}
static void pinned_give(znippy_ctx *ctx, void *p, size_t cap) {
    if (!p) return;
    if (ctx->pinned_pool.size() < 16 && ctx->pinned_pool_bytes + cap <= (256ull << 20)) {
        ctx->pinned_pool.emplace_back(cap, p);
        ctx->pinned_pool_bytes += cap;
    } else (void)hipHostFree(p);
}
// Events of tables (two or four each) come from a per-context free list: creating one costs ~0.1 ms.
static hipEvent_t event_take(znippy_ctx *ctx) {
    if (!ctx->event_pool.empty()) {
        hipEvent_t e = ctx->event_pool.back();
        ctx->event_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
    return e;
}
static void event_give(znippy_ctx *ctx, hipEvent_t e) {
    if (!e) return;
    if (ctx->event_pool.size() < 64) ctx->event_pool.push_back(e);
    else (void)hipEventDestroy(e);
}

// ---- run lanes: what every entry point and every run that is not a lane run does first ----------------------------------
// The main stream gets behind every lane run queued so far, and the next lane run will get behind the main stream.
static void lanes_close(znippy_ctx *ctx) {
    if (!ctx->lanes_on) return;
    if (ctx->lane_join) { (void)hipStreamWaitEvent(ctx->stream, ctx->lane_join, 0); ctx->lane_join = nullptr; }
    ctx->main_dirty = true; ctx->mark_pending = false;
    ctx->lane_prev.valid = false;  // (the main stream, and with it the mark the next lane run stands behind, is behind every lane run)
    for (auto &h : ctx->lane_hist) h[0].valid = h[1].valid = false;
}
static hipError_t lanes_sync(znippy_ctx *ctx) { return ctx->lane ? hipStreamSynchronize(ctx->lane) : hipSuccess; }
// Opens every public entry point that takes a context: false = the context was destroyed and is only kept alive by its tables
// (every call fails with ZNIPPY_E_INVAL).  ENTER_WORK: the call may queue work on the main stream, so the lanes are closed
// first — an entry point written after this pattern is ordered against the lane runs without knowing of them.  ENTER_RUN:
// the async run calls and the results calls, whose every stream operation goes through rows_launch: that closes the lanes
// itself unless the run is a lane run, and a results call that repeats nothing queues nothing.  ENTER_HOST: calls that read
// or set host state only (levels, kernel timing, the last kernel times) and can never queue or wait for device work.
enum EnterKind { ENTER_WORK, ENTER_RUN, ENTER_HOST };
static inline bool ctx_enter(znippy_ctx *ctx, EnterKind kind = ENTER_WORK) {
    if (!ctx) return true;  // (the null check and its return value are the entry point's own)
    if (ctx->closing) return false;
    if (kind == ENTER_WORK) lanes_close(ctx);
    return true;
}

// Device memory of the tables (index columns, plans, per-run scratch) comes from a per-context pool: a table is
// built and torn down per hand-off in the host pipelines, and ~15 hipMalloc + hipFree pairs cost more than the
// kernels of a small hand-off.  Nothing in a table relies on fresh memory: every array is either uploaded, reset by
// the run (memset) or written before it is read (DESIGN.md §3a lists which, array by array; ZNIPPY_POISON tests it).
template <class T>
static hipError_t tmalloc(znippy_ctx *ctx, T **out, size_t bytes) {
    bytes = std::max<size_t>(bytes, 16);
    size_t best = ctx->dev_pool.size();
    for (size_t i = 0; i < ctx->dev_pool.size(); i++)
        if (ctx->dev_pool[i].first >= bytes && ctx->dev_pool[i].first <= 2 * bytes + 4096 &&
            (best == ctx->dev_pool.size() || ctx->dev_pool[i].first < ctx->dev_pool[best].first))
            best = i;
    if (best != ctx->dev_pool.size()) {
        *out = (T *)ctx->dev_pool[best].second;
        ctx->dev_sizes[*out] = ctx->dev_pool[best].first;
        ctx->dev_pool_bytes -= ctx->dev_pool[best].first;
        ctx->dev_pool.erase(ctx->dev_pool.begin() + best);
        return ctx->sw.poison ? poison_dev(ctx, *out, ctx->dev_sizes[*out]) : hipSuccess;  // (the whole capacity, not only `bytes`)
    }
    void *p = nullptr;
    const hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) return e;
    *out = (T *)p;
    ctx->dev_sizes[p] = bytes;
    return ctx->sw.poison ? poison_dev(ctx, p, bytes) : hipSuccess;
}
static void tfree(znippy_ctx *ctx, void *p) {
    if (!p) return;
    auto it = ctx->dev_sizes.find(p);
    if (it == ctx->dev_sizes.end()) { (void)hipFree(p); return; }
    const size_t cap = it->second;
    ctx->dev_sizes.erase(it);
    if (ctx->dev_pool.size() < 96 && ctx->dev_pool_bytes + cap <= (1ull << 30)) {
        ctx->dev_pool.emplace_back(cap, p);
        ctx->dev_pool_bytes += cap;
    } else (void)hipFree(p);
}
// Up to two tmalloc'ed buffers of a call that go back to the pool when the call returns — once the main stream has run whatever is
// still queued on them.
template <class A, class B = void>
struct SyncFree {
    znippy_ctx *ctx;
    A *a = nullptr;
    B *b = nullptr;
    ~SyncFree() {
        if (!a && !b) return;
        (void)hipStreamSynchronize(ctx->stream);
        tfree(ctx, a); tfree(ctx, b);
    }
};

struct DevPlan {
    Tile *tiles = nullptr;
    BigUnit *big = nullptr;
    uint32_t *tile_cv = nullptr;
    uint32_t *grp_big = nullptr, *grp_k = nullptr;
    uint32_t n_grp = 0;
    uint32_t n_tiles = 0, n_big = 0;
    uint32_t max_cvs = 0;  // tile CVs of the biggest unit (picks the merge launch)
};

static int upload_plan(znippy_ctx *ctx, const PlanBuf &p, DevPlan &d) {
    d.n_tiles = (uint32_t)p.tiles.size();
    d.n_big = (uint32_t)p.big.size();
    d.max_cvs = plan_max_cvs(p);
    if (d.n_tiles) {
        HIPCHK(ctx, tmalloc(ctx, &d.tiles, sizeof(Tile) * d.n_tiles));
        HIPCHK(ctx, hipMemcpy(d.tiles, p.tiles.data(), sizeof(Tile) * d.n_tiles, hipMemcpyHostToDevice));
    }
    if (d.n_big) {
        HIPCHK(ctx, tmalloc(ctx, &d.big, sizeof(BigUnit) * d.n_big));
        HIPCHK(ctx, hipMemcpy(d.big, p.big.data(), sizeof(BigUnit) * d.n_big, hipMemcpyHostToDevice));
        HIPCHK(ctx, tmalloc(ctx, &d.tile_cv, 32 * ((size_t)p.n_tile_cv + p.grp_big.size())));
        d.n_grp = (uint32_t)p.grp_big.size();
        if (d.n_grp) {
            HIPCHK(ctx, tmalloc(ctx, &d.grp_big, 4 * (size_t)d.n_grp));
            HIPCHK(ctx, tmalloc(ctx, &d.grp_k, 4 * (size_t)d.n_grp));
            HIPCHK(ctx, hipMemcpy(d.grp_big, p.grp_big.data(), 4 * (size_t)d.n_grp, hipMemcpyHostToDevice));
            HIPCHK(ctx, hipMemcpy(d.grp_k, p.grp_k.data(), 4 * (size_t)d.n_grp, hipMemcpyHostToDevice));
        }
    }
    return ZNIPPY_OK;
}

static void free_plan(znippy_ctx *ctx, DevPlan &d) {
    tfree(ctx, d.tiles);
    tfree(ctx, d.big);
    tfree(ctx, d.tile_cv);
    tfree(ctx, d.grp_big);
    tfree(ctx, d.grp_k);
    d = DevPlan();
}

// The control block of a row table (znippy_rows::ctl): ONE allocation, cleared (or preset from status_init) by ONE stream
// operation per run.  The regions below, then from CTL_HEAD on the status column (n x i32).  The first CTL_MIRROR bytes
// travel to the host mirror (h_counters) behind every run.
struct CtlRegion { size_t at, bytes; };
constexpr CtlRegion CTL_COUNTERS{0, 8 * 8};    // u64: k_verify's counters; [CTL_FLAG] != 0: a lean run left something on a list (rows_settle)
constexpr CtlRegion CTL_HAND{64, 16 * 4};      // u32: hand-over counts, indexed by Hand
constexpr CtlRegion CTL_CURSORS{128, 16 * 4};  // u32: work cursors, indexed by Cursor
constexpr CtlRegion CTL_FZ_POOL{192, 8 * 8};   // u64: pool counters of the two-phase path (FzArgs::pool_used)
constexpr CtlRegion CTL_BX_POOL{256, 16 * 8};  // u64: pool counters of the batch path (BxArgs::pool_used)
constexpr CtlRegion CTL_BX_CTR{384, 16 * 4};   // u32: its work counters (BxArgs::ctr)
constexpr CtlRegion CTL_RX{448, 16 * 4};       // u32: words left after each resolve round (BxArgs::rx_pending, RX_ROUNDS of them); [RX_ZERO] is never written
constexpr CtlRegion CTL_BX_XXH{512, 4 * 8};    // u64: the checksum stage's counters (BxArgs::xxh_stat, znippy_rows_checksum_stats)
constexpr size_t CTL_HEAD = 768, CTL_MIRROR = 128, CTL_FLAG = 7;  // (the status column keeps the 256-byte alignment it had at 512)
constexpr uint32_t RX_ZERO = 15;
enum Hand : uint32_t {  // length of a list one kernel leaves to another; the mirror tells the next run's plan which were empty
    H_FUSED = 0,    // rows handed over by the fused kernels (pending)
    H_SERIAL = 1,   // rows for the serial decoder (pending2)
    H_ITEMS = 2,    // block items left by the fused block kernel (todo)
    H_TILES = 3,    // tiles left by the role-split kernel (slow_list)
    H_FLAGGED = 5,  // block candidates left flagged for the batch path: k_finish_blocks counts them at ITS pending_count (H_SERIAL) + 4
};
enum Cursor : uint32_t { CUR_GENERAL = 0, CUR_ROLES = 2, CUR_ITEMS = 4, CUR_FALLBACK = 8, CUR_FZ = 12, CUR_FZ_WORK = 13 };  // CUR_FZ_WORK: the two-phase path's work count
// the lists a lean run must have left empty (k_verify's mask over the hand-over counts): small rows / big multi-block rows
constexpr uint32_t LEAN_ANY = 1u << H_FUSED | 1u << H_SERIAL | 1u << H_FLAGGED, LEAN_SMALL = LEAN_ANY | 1u << H_TILES, LEAN_BLOCKS = LEAN_ANY | 1u << H_ITEMS;
constexpr bool ctl_before(CtlRegion a, CtlRegion b) { return a.at + a.bytes <= b.at; }
static_assert(ctl_before(CTL_COUNTERS, CTL_HAND) && ctl_before(CTL_HAND, CTL_CURSORS) && ctl_before(CTL_CURSORS, CTL_FZ_POOL) && ctl_before(CTL_FZ_POOL, CTL_BX_POOL) &&
              ctl_before(CTL_BX_POOL, CTL_BX_CTR) && ctl_before(CTL_BX_CTR, CTL_RX) && ctl_before(CTL_RX, CTL_BX_XXH) && CTL_BX_XXH.at + CTL_BX_XXH.bytes <= CTL_HEAD && CTL_HEAD % 256 == 0,
              "control block: regions overlap or pass the head");
static_assert(CTL_COUNTERS.at == 0 && CTL_HAND.at == CTL_COUNTERS.bytes && CTL_MIRROR == CTL_HAND.at + CTL_HAND.bytes, "the mirror is exactly counters + hand-over counts");
static_assert(CTL_FLAG < 8 && H_FLAGGED == H_SERIAL + 4 && H_FLAGGED < 8 && CUR_FZ_WORK < 16 && zn::RX_ROUNDS <= RX_ZERO && RX_ZERO < 16, "control block: a word outside its region");

struct znippy_rows {
    znippy_ctx *ctx = nullptr;
    uint64_t row_begin = 0;
    RowsShape shape;  // what creation learnt about the rows (host/rows_plan.h: rows_classify)
    RowsHints hints;  // what the last finished run and the host's validation left (rows_note_hint, rows_validate)
    uint64_t *blob_off = nullptr, *blob_size = nullptr, *usize = nullptr, *out_off = nullptr;
    uint8_t *compressed = nullptr, *checksum = nullptr, *d_bitmap = nullptr;
    uint32_t *h_pack = nullptr, *d_pack = nullptr;  // front-to-back tables: the two size columns as 32-bit values (page-locked / device)
    size_t h_pack_cap = 0;
    unsigned long long *d_pack_sums = nullptr;
    uint8_t *ctl = nullptr;  // the control block (layout: CtlRegion above)
    size_t ctl_bytes = 0;
    template <class T> T *ctl_at(CtlRegion g, size_t i = 0) const { return reinterpret_cast<T *>(ctl + g.at) + i; }
    uint32_t *hand(Hand h) const { return ctl_at<uint32_t>(CTL_HAND, h); }
    uint32_t *cur(Cursor c) const { return ctl_at<uint32_t>(CTL_CURSORS, c); }
    int32_t *status = nullptr;
    uint32_t *digests = nullptr;
    uint64_t *counters = nullptr;
    // Two slots of the per-run device state, like the mirror below: run k owns control block, digest column and corrupt list
    // k & 1, so the verify of run k need not stand between the main kernels of run k and run k + 1 (run_verify).  ctl,
    // status, counters, digests and corrupt above are the slot of the run queued LAST (select: rows_launch, behind the run's
    // allocations), which is what the "latest run" outputs read and what a run's stages are given.
    uint8_t *ctl_m[2] = {nullptr, nullptr};
    uint32_t *digests_m[2] = {nullptr, nullptr};
    uint64_t *corrupt_m[2] = {nullptr, nullptr};
    void select(unsigned slot) {
        ctl = ctl_m[slot]; digests = digests_m[slot]; corrupt = corrupt_m[slot];
        counters = ctl_at<uint64_t>(CTL_COUNTERS);
        status = reinterpret_cast<int32_t *>(ctl + CTL_HEAD);
    }
    hipEvent_t ev_main[2] = {nullptr, nullptr};  // forked verify: the end of the run's kernels on the main stream
    bool lane_used = false;  // a run of this table was ever queued on the context's run lane (the same parties wait for that stream)
    bool aux_used = false;  // a verify of this table was ever queued on the auxiliary stream (whoever reuses a slot or frees the table joins it)
    // pinned mirror of the counters, filled by the run's own D2H copy.  Two slots + one event each: run k uses slot
    // k & 1, so the counters of run k can be read while run k + 1 is already executing (znippy_rows_results_lagged)
    uint64_t *h_counters = nullptr;  // per slot CTL_MIRROR bytes (16 x u64): the counters, then the 16 hand-over counts (u32)
    HandCounts mirror_hand(unsigned slot) const {  // the hand-over counts a finished run left in its mirror slot
        const uint32_t *left = reinterpret_cast<const uint32_t *>(reinterpret_cast<const uint8_t *>(h_counters + 16 * slot) + CTL_HAND.at);
        return HandCounts{left[H_FUSED], left[H_SERIAL], left[H_FLAGGED], left[H_TILES], left[H_ITEMS]};
    }
    size_t h_counters_cap = 0;
    uint32_t *all_rows = nullptr;  // RowsHints::small_off: the batch path's list of every row (made by the first run that needs it)
    struct RunArgs { const void *blobs = nullptr; void *out = nullptr; uint64_t base = 0, cap = 0, blob_cap = ~0ull; bool verify = false, plain = false; } run_args[2];  // per mirror slot: what the run was given, and its kind (plain: decode-only)
    // verify-only runs: the second output column — a 16-byte aligned slot in the context's scratch for every compressed row with bytes
    // (stored rows and empty rows: none) — built on the device at the table's first verify run; vs_bytes = the slots' extent
    uint64_t *vs_off = nullptr;
    uint64_t vs_bytes = 0;
    bool vs_built = false;
    bool no_out = false;  // created without output offsets: the table can only be verified
    hipEvent_t ev_done[2] = {nullptr, nullptr};
    uint64_t run_seq = 0;  // async runs queued so far
    // Host copies of the columns a run is validated against (one pass per distinct (blob_base, blob_cap, out_cap)):
    // a row whose blob lies outside the blob region, or whose bytes would land outside the output region, gets its
    // status from the host (status_init) and no kernel touches it — a crafted index is an error code, not a fault.
    // A run whose regions contain the table's extents has no bad row; otherwise the columns come back from the device for
    // the per-row pass (h_*: filled then)
    std::vector<uint64_t> h_blob_off, h_blob_size, h_len, h_out_off;
    std::vector<uint8_t> h_comp;  // range reads: the byte-per-row flags beside the three columns above (rows_host_columns)
    uint64_t blob_cap = ~0ull;  // size of the caller's blob region (znippy_rows_set_blob_cap); ~0 = not declared
    // block tree (znippy_rows_set_block_tree): the layout (n + 1 first-entry numbers, filled at first use), a device copy of the
    // installed entries, which rows' entries fold to their checksum (accepted), and a host copy of the checksum column
    std::vector<uint64_t> tree_first;
    uint32_t *tree_dev = nullptr;
    std::vector<uint8_t> tree_accept;
    std::vector<uint8_t> h_checksum;
    uint64_t val_base = 0, val_bcap = 0, val_ocap = 0;
    bool val_done = false, val_verify = false;
    uint8_t *status_init = nullptr;  // image of ctl with the host-decided statuses (rows_validate)
    uint64_t *corrupt = nullptr;
    uint32_t corrupt_cap = 0;
    uint32_t *list_a = nullptr;   // compressed rows with > 64 leaves: general decoder
    uint32_t *pending = nullptr;  // rows the fused kernel hands over (count: H_FUSED)
    // block items: compressed rows of >= 2 blocks are tried block by block first
    uint32_t *cand_row = nullptr, *cand_base = nullptr, *cand_nblocks = nullptr, *pending2 = nullptr;
    // two-phase path for the candidates the block-item path gives up on (foreign frames): item slots per candidate, the work list of the run
    uint32_t *fz_base = nullptr, *fz_cap = nullptr, *fz_it_cand = nullptr, *fz_nb = nullptr, *fz_work = nullptr;
    zn::FzItem *fz_items = nullptr;
    // batch path (k_bx_*): candidate slots (one per compressed row at most), item slots, the two entropy work lists
    uint32_t *bx_cand_ck = nullptr;  // checksum stage: which slots hold a frame with a trailer (allocated by the first run with the switch on)
    uint32_t *bx_cand_row = nullptr, *bx_cand_base = nullptr, *bx_cand_nb = nullptr, *bx_huf_list = nullptr, *bx_seq_list = nullptr, *bx_sort_tmp = nullptr;
    zn::FzItem *bx_items = nullptr;
    zn::BxPrep *bx_prep = nullptr;
    uint32_t *rx_base = nullptr, *rx_fail = nullptr, *rx_blk = nullptr, *rx_list = nullptr;  // resolve path
    uint32_t *item_row = nullptr, *item_k = nullptr, *item_src = nullptr, *row_flag = nullptr;
    // fused block kernel: big-slice tiles of the candidate rows, the item each belongs to, and what it got done
    uint32_t *bt_tile = nullptr, *bt_item = nullptr;
    uint8_t *tile_done = nullptr, *item_done = nullptr;  // one allocation (item_done lies behind tile_done)
    size_t done_bytes = 0;
    uint32_t *todo = nullptr;  // items left to the block decoder (count: H_ITEMS)
    uint32_t *slow_list = nullptr;  // tiles the role-split kernel leaves to k_fused_small (count: H_TILES)
    DevPlan plan;
};

struct znippy_rounds {
    znippy_ctx *ctx = nullptr;
    uint32_t n = 0;
    uint64_t *src_off = nullptr, *len = nullptr;
    uint8_t *skip = nullptr;
    std::vector<uint8_t> h_skip;  // empty: no round is a store-path round
    void *plan_scratch[3] = {nullptr, nullptr, nullptr};  // per-round prefix sums of the plan kernels (freed with the table)
    uint64_t in_bytes = 0, enc_bytes = 0;  // all rounds / rounds that go through the encoder
    bool all_stored_aligned = false;       // every round is a skip round and every blob offset will be a multiple of 16
    uint64_t blob_bound = 0;
    DevPlan plan;
    // encoder plan: one item per output piece
    EncItem *items = nullptr;
    uint32_t n_items = 0;
    // Encoder variant per block, by the block's own length (so a round's frame does not depend on what else is
    // in the batch): blocks <= 16 KiB go to the small-table variant (more waves), the rest to the wide one.
    // order_*: item indices of each share; NULL when the whole plan is of one kind.
    uint32_t *order_small = nullptr, *order_wide = nullptr;
    uint32_t n_small = 0, n_wide = 0;
    uint32_t *retry_list = nullptr, *retry_count = nullptr;  // small blocks the small variant hands to the wide one
    uint64_t prov_bytes = 0;
    uint32_t *piece_len = nullptr, *piece_len_init = nullptr;
    uint64_t *piece_start = nullptr, *local_excl = nullptr, *block_tot = nullptr;
    // results live in ONE device slab (one copy out per call: ResSlab)
    // Two slabs + two mirrors + one event each: run k uses slot k & 1 and its copy rides the context's copy
    // stream, so run k + 1 encodes while run k's results travel (and are read: znippy_rounds_results_lagged).
    uint8_t *res_m[2] = {nullptr, nullptr}, *h_res_m[2] = {nullptr, nullptr};  // device slabs + their pinned host mirrors
    unsigned slot = 0;  // of the run queued last (0 before the first): znippy_rounds_results reads it, znippy_hash_rounds writes its digests
    ResSlab dev(unsigned k) const { return ResSlab{res_m[k], n}; }
    ResSlab host(unsigned k) const { return ResSlab{h_res_m[k], n}; }
    size_t h_res_cap_m[2] = {0, 0}, h_stored_cap = 0;
    hipEvent_t ev_enc[2] = {nullptr, nullptr}, ev_res[2] = {nullptr, nullptr};
    uint64_t run_seq = 0;
    size_t res_bytes = 0;
    bool store_incompressible = false;  // opt-in (znippy_rounds_set_store_incompressible)
    int fuse_tiles = 0;  // > 0: every round is a small encoded round (one block, no store path): the encoder hashes its tiles itself, this many per dequeue
    uint32_t *first_item = nullptr;     // first piece of every round
    uint32_t blob_align = 1;            // opt-in (znippy_rounds_set_blob_align): every blob offset is a multiple of it
    uint32_t *piece_pad = nullptr;      // zero bytes behind every piece (made by the first alignment above 1; only the rounds' last pieces are ever written)
    uint8_t *stored = nullptr, *h_stored = nullptr;  // per round: turned into a raw payload by the opt-in pass
    // far window: the rounds longer than one block and their regions of the index (found at creation; the device copies
    // are made by the first windowed encode call)
    std::vector<LdmRound> h_ldm;
    uint64_t ldm_entries = 0;
    uint32_t ldm_chunks = 0;
    LdmRound *d_ldm = nullptr;
    uint64_t *d_ldm_desc = nullptr;  // per round: its region (LDM_NONE: not indexed)
    // block tree (opt-in, znippy_rounds_emit_block_tree): the runs queued while it is on leave their entries in the slot's buffer
    bool emit_tree = false;
    bool tree_run[2] = {false, false};  // the run in this slot was queued with emission on
    std::vector<uint64_t> tree_first;   // round i's entries are [tree_first[i], tree_first[i + 1]) (made by the first call that asks)
    TreeUnit *tree_units = nullptr;     // the big units with entries + a sentinel (made by the first switch-on, as everything below)
    uint32_t n_tree_units = 0, n_tree_entries = 0;
    bool tree_ready = false;
    uint32_t *tree_m[2] = {nullptr, nullptr};
    uint8_t *h_tree_m[2] = {nullptr, nullptr};
    size_t h_tree_cap_m[2] = {0, 0};
};

// ------------------------------------------------------------------------------------------------
static bool ktime_on(const znippy_ctx *ctx, const char *name) {
    return ctx->sw.ktime >= 2 || (ctx->sw.ktime == 1 && (!strncmp(name, "decode_verify_", 14) || !strncmp(name, "verify_", 7)));
}
static void ktime_begin(znippy_ctx *ctx, const char *name, hipStream_t on = nullptr) {
    if (ctx->sw.trace) { fprintf(stderr, "[znippy trace] %s ...", name); fflush(stderr); }
    ctx->ktime_open = ktime_on(ctx, name);
    if (!ctx->ktime_open) return;
    if ((int)ctx->ktimes.size() <= ctx->n_ktimes) {
        KTime k{name, nullptr, nullptr};
        (void)hipEventCreate(&k.t0);
        (void)hipEventCreate(&k.t1);
        ctx->ktimes.push_back(k);
    }
    ctx->ktimes[ctx->n_ktimes].name = name;
    (void)hipEventRecord(ctx->ktimes[ctx->n_ktimes].t0, on ? on : ctx->stream);
}
static void ktime_end(znippy_ctx *ctx, hipStream_t on = nullptr) {
    if (ctx->sw.trace) {  // diagnosis of a faulting launch: every bracketed launch runs to its end before the next starts
        const hipError_t e = hipStreamSynchronize(on ? on : ctx->stream);
        fprintf(stderr, " %s\n", e == hipSuccess ? "done" : hipGetErrorString(e));
        fflush(stderr);
    }
    if (!ctx->ktime_open) return;
    (void)hipEventRecord(ctx->ktimes[ctx->n_ktimes].t1, on ? on : ctx->stream);
    ctx->n_ktimes++;
}

// one bracketed launch (the callable is inlined: no allocation, nothing virtual on the 0.5 ms step)
template <class F>
static inline void timed(znippy_ctx *ctx, const char *name, hipStream_t on, F &&launch) {
    ktime_begin(ctx, name, on);
    launch();
    ktime_end(ctx, on);
}
// Diagnostic stamps of a kernel kind (N words, in the context: allocated at first use on ITS device, freed with it).  Waits for
// the given streams (s1 may be null), hands the previous launch's stamps to `print`, clears them and returns the device buffer
// for the next launch's argument struct.
template <size_t N, class Print>
static unsigned long long *diag_cycle(znippy_ctx *ctx, znippy_ctx::Diag which, hipStream_t s0, hipStream_t s1, Print print) {
    unsigned long long *&d = ctx->diag[which];
    if (!d) { (void)hipMalloc(&d, 8 * N); (void)hipMemset(d, 0, 8 * N); }
    unsigned long long h[N];
    (void)hipStreamSynchronize(s0);
    if (s1) (void)hipStreamSynchronize(s1);
    (void)hipMemcpy(h, d, 8 * N, hipMemcpyDeviceToHost);
    print(h);
    (void)hipMemset(d, 0, 8 * N);
    return d;
}

// what the caller gave a run; preset != 0: the status column starts as the host's verdicts (rows_validate found bad rows); slot: its mirror slot and event
// verify: a verify-only run — d_out / out_cap are the context's scratch and the extent of the table's slots in it, and the output column is vs_off
// plain: a decode-only run (znippy_decode_rows) — rows are written as in a decode run and nothing is hashed
// on: the stream of the run's main chain — the context's main stream, or for a lean run on lane 1 the run lane (lane_begin)
struct RowsRun { const void *d_blobs; uint64_t blob_base; void *d_out; uint64_t out_cap; int preset; unsigned slot; bool verify; bool plain; hipStream_t on; hipEvent_t lane_ev; };
// the ten row columns every decode path's argument struct has under the same names (BlockScanArgs: all but `out`)
static void set_out(BlockScanArgs &, uint8_t *) {}
template <class A> static void set_out(A &a, uint8_t *out) { a.out = out; }
template <class A>
static void fill_row_args(A &a, const znippy_rows *r, const RowsRun &run) {
    a.blobs = (const uint8_t *)run.d_blobs; a.blob_base = run.blob_base;
    a.blob_off = r->blob_off; a.blob_size = r->blob_size; a.usize = r->usize; a.out_off = run.verify ? r->vs_off : r->out_off;
    a.out_cap = run.out_cap; a.status = r->status; a.preset = run.preset;
    set_out(a, (uint8_t *)run.d_out);
}

template <class T>
static int dev_upload(znippy_ctx *ctx, T **d, const T *h, size_t n) {
    HIPCHK(ctx, tmalloc(ctx, d, sizeof(T) * n));
    if (n) HIPCHK(ctx, hipMemcpy(*d, h, sizeof(T) * n, hipMemcpyHostToDevice));
    return ZNIPPY_OK;
}

// Scratch that only one side of the path needs is allocated on that side's first call (a verify-only context
// never pays for the encoder's 400 MB of sequence scratch, nor an encode-only one for the literal scratch).
static int ensure_decoder(znippy_ctx *ctx) {
    if (ctx->lit_scratch) return ZNIPPY_OK;
    if (hipMalloc(&ctx->lit_scratch, decode_lit_scratch_bytes(ctx->decode_grid)) != hipSuccess) return ZNIPPY_E_NOMEM;
    if (ctx->sw.poison) (void)poison_dev(ctx, ctx->lit_scratch, decode_lit_scratch_bytes(ctx->decode_grid));
    return ZNIPPY_OK;
}
// the block-item launches' literal scratch (they run beside the general decoder): made by the first run or range call that has block items
static int ensure_decoder_b(znippy_ctx *ctx) {
    if (ctx->lit_scratch_b) return ZNIPPY_OK;
    if (hipMalloc(&ctx->lit_scratch_b, decode_lit_scratch_bytes(ctx->decode_grid)) != hipSuccess) { (void)hipGetLastError(); ctx->lit_scratch_b = nullptr; return ZNIPPY_E_NOMEM; }
    if (ctx->sw.poison) (void)poison_dev(ctx, ctx->lit_scratch_b, decode_lit_scratch_bytes(ctx->decode_grid));
    return ZNIPPY_OK;
}
// One grow-only pool of the context (sizes: host/rows_plan.h): when `want` is more than it holds, the main stream is waited for
// (runs in flight use the pool: the auxiliary streams have joined by the end of a run), its buffers are freed and made again.
// false: no memory — nothing is left of the pool, which an optional one's users take as "no pool" and a required one's as
// ZNIPPY_E_NOMEM.
struct PoolBuf { void **p; uint64_t bytes; };
static bool pool_grow(znippy_ctx *ctx, std::initializer_list<PoolBuf> bufs, uint64_t *cap, uint64_t want) {
    if (want <= *cap) return true;
    (void)hipStreamSynchronize(ctx->stream);
    for (const PoolBuf &b : bufs) { if (*b.p) (void)hipFree(*b.p); *b.p = nullptr; }
    *cap = 0;
    for (const PoolBuf &b : bufs)
        if (hipMalloc(b.p, b.bytes) != hipSuccess) {
            (void)hipGetLastError();
            *b.p = nullptr;
            for (const PoolBuf &f : bufs) { if (*f.p) (void)hipFree(*f.p); *f.p = nullptr; }
            return false;
        }
    *cap = want;
    if (ctx->sw.poison)
        for (const PoolBuf &b : bufs) (void)poison_dev(ctx, *b.p, b.bytes);
    return true;
}
// the two-phase path's pools; without one of them the serial decoder keeps the frames
static int ensure_fz_pools(znippy_ctx *ctx, uint64_t content_bytes, uint32_t items) {
    const FzPoolSizes z = fz_pool_sizes(content_bytes, items);
    if (pool_grow(ctx, {{(void **)&ctx->fz_lit_pool, z.lit_bytes}}, &ctx->fz_lit_cap, z.lit_bytes))
        (void)pool_grow(ctx, {{(void **)&ctx->fz_seq_pool, z.seq_records * 8}}, &ctx->fz_seq_cap, z.seq_records);
    return ZNIPPY_OK;
}
// the batch path's table pools, the predefined tables at the head of the FSE pool
static int ensure_bx_pools(znippy_ctx *ctx, uint64_t content_bytes, uint32_t items) {
    const BxPoolSizes z = bx_pool_sizes(content_bytes, items);
    const uint64_t had = ctx->bx_fse_cap;
    if (!pool_grow(ctx, {{(void **)&ctx->bx_fse_pool, z.fse_cells * 2}}, &ctx->bx_fse_cap, z.fse_cells)) return ZNIPPY_OK;
    if (ctx->bx_fse_cap != had) {
        uint16_t predef[BX_POOL_FIRST];
        bx_predefined_tables(predef);
        if (hipMemcpy(ctx->bx_fse_pool, predef, sizeof predef, hipMemcpyHostToDevice) != hipSuccess) { ctx->bx_fse_cap = 0; return ZNIPPY_E_HIP; }
    }
    (void)pool_grow(ctx, {{(void **)&ctx->bx_huf_pool, z.huf_cells * 2}}, &ctx->bx_huf_cap, z.huf_cells);
    return ZNIPPY_OK;
}
// the resolve path's word pool with its chunk tables (hipMalloc of 8 GiB takes 0.3 ms on this system); no pool: the frames are
// executed by a wave each
static int ensure_rx_pool(znippy_ctx *ctx, uint64_t words) {
    words = rx_pool_words(words);
    (void)pool_grow(ctx, {{(void **)&ctx->rx_pool, words * 4}, {(void **)&ctx->rx_chunk, words / 1024 * 4}, {(void **)&ctx->rx_cdone, words / 1024}}, &ctx->rx_cap, words);
    return ZNIPPY_OK;
}
// the verify-only runs' scratch and the range reads' two regions: not optional — a call that needs more than may be had is refused
static int ensure_scratch(znippy_ctx *ctx, uint8_t **pool, uint64_t *cap, uint64_t bytes) {
    if (bytes == POOL_REFUSED) return ZNIPPY_E_NOMEM;
    return pool_grow(ctx, {{(void **)pool, bytes}}, cap, bytes) ? ZNIPPY_OK : ZNIPPY_E_NOMEM;
}
static int ensure_verify_scratch(znippy_ctx *ctx, uint64_t bytes) { return ensure_scratch(ctx, &ctx->vs_pool, &ctx->vs_cap, verify_scratch_bytes(bytes)); }
static int ensure_range_scratch(znippy_ctx *ctx, int which, uint64_t bytes) {
    return ensure_scratch(ctx, &ctx->rr_pool[which], &ctx->rr_cap[which], range_scratch_bytes(bytes, ctx->rr_cap[which ^ 1]));
}
static int ensure_encoder(znippy_ctx *ctx) {
    if (ctx->enc_tabs) return ZNIPPY_OK;
    EncTables t;
    build_encode_tables(&t);
    if (hipMalloc(&ctx->enc_seq, (size_t)ctx->encode_grid * MAX_SEQ * 3 * 4) != hipSuccess ||
        hipMalloc(&ctx->enc_tabs, sizeof(EncTables)) != hipSuccess ||
        hipMemcpy(ctx->enc_tabs, &t, sizeof t, hipMemcpyHostToDevice) != hipSuccess) {
        if (ctx->enc_tabs) { (void)hipFree(ctx->enc_tabs); ctx->enc_tabs = nullptr; }
        return ZNIPPY_E_NOMEM;
    }
    if (ctx->sw.poison) (void)poison_dev(ctx, ctx->enc_seq, (size_t)ctx->encode_grid * MAX_SEQ * 3 * 4);
    return ZNIPPY_OK;
}

// ZNIPPY_POISON: every pool and scratch buffer of the context filled again, at the start of an entry point that queues a run or a
// batch call — after everything the context has queued anywhere has ended (a debug mode: the runs of a pipeline no longer
// overlap; their results may not change).  A call made from inside another one (the private runs of a range read, the runs
// behind the single-chunk shims' staging) finds the hold set and leaves the pools as the outer call has them.
// Kept, because they are written once and read by every later run:
//  - the predefined tables at the head of bx_fse_pool (BX_POOL_FIRST cells, uploaded when the pool is made or grown);
//  - enc_tabs (uploaded when the encoder's scratch is made) — not in the list at all;
//  - shim_in / shim_out: the single-chunk shims stage the caller's bytes there BEFORE the run they queue (filled when allocated only);
//  - clk_buf and diag[]: diagnostics that add up over launches, zeroed where they are made.
// Everything else a run or call finds in a pool it must have written itself (DESIGN.md §3a lists who does).
static int poison_pools(znippy_ctx *ctx) {
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, lanes_sync(ctx));
    if (ctx->aux) HIPCHK(ctx, hipStreamSynchronize(ctx->aux));
    if (ctx->copy) HIPCHK(ctx, hipStreamSynchronize(ctx->copy));
    const size_t lit = decode_lit_scratch_bytes(ctx->decode_grid), head = sizeof(uint16_t) * BX_POOL_FIRST;
    const struct { void *p; size_t from, bytes; } pools[] = {
        {ctx->lit_scratch, 0, lit}, {ctx->lit_scratch_b, 0, lit},
        {ctx->fz_lit_pool, 0, (size_t)ctx->fz_lit_cap}, {ctx->fz_seq_pool, 0, (size_t)ctx->fz_seq_cap * 8},
        {ctx->bx_fse_pool, head, (size_t)ctx->bx_fse_cap * 2}, {ctx->bx_huf_pool, 0, (size_t)ctx->bx_huf_cap * 2},
        {ctx->rx_pool, 0, (size_t)ctx->rx_cap * 4}, {ctx->rx_chunk, 0, (size_t)(ctx->rx_cap / 1024) * 4}, {ctx->rx_cdone, 0, (size_t)(ctx->rx_cap / 1024)},
        {ctx->vs_pool, 0, (size_t)ctx->vs_cap}, {ctx->rr_pool[0], 0, (size_t)ctx->rr_cap[0]}, {ctx->rr_pool[1], 0, (size_t)ctx->rr_cap[1]},
        {ctx->enc_seq, 0, (size_t)ctx->encode_grid * MAX_SEQ * 3 * 4}, {ctx->enc_prov, 0, ctx->enc_prov_cap}, {ctx->ldm, 0, 4 * ctx->ldm_cap},
        {ctx->cursor, 0, 64},
    };
    for (const auto &b : pools)
        if (b.p && b.bytes > b.from) HIPCHK(ctx, hipMemsetAsync((uint8_t *)b.p + b.from, ctx->sw.poison_byte, b.bytes - b.from, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return ZNIPPY_OK;
}
static inline int poison_enter(znippy_ctx *ctx) { return ctx->sw.poison && !ctx->poison_hold ? poison_pools(ctx) : ZNIPPY_OK; }
struct PoisonHold {  // the scope of an entry point whose inner calls must find the pools as it left them
    znippy_ctx *ctx;
    explicit PoisonHold(znippy_ctx *c) : ctx(c->sw.poison ? c : nullptr) { if (ctx) ctx->poison_hold++; }
    ~PoisonHold() { if (ctx) ctx->poison_hold--; }
    PoisonHold(const PoisonHold &) = delete;
    PoisonHold &operator=(const PoisonHold &) = delete;
};

// rows of a front-to-back table arrive as two 32-bit size columns (zn_rows_pack32): the four 64-bit columns the kernels read
// are made here — sizes widened, offsets = first offset + running sum (per 1,024 rows: sums, their scan, fill)
__device__ __forceinline__ void block_excl_scan2(unsigned long long &a, unsigned long long &b, unsigned long long *sa, unsigned long long *sb,
                                                 unsigned long long *ta, unsigned long long *tb) {  // 256 threads: exclusive sums + totals
    const uint32_t t = threadIdx.x;
    const unsigned long long a0 = a, b0 = b;
    sa[t] = a; sb[t] = b;
    __syncthreads();
    for (uint32_t d = 1; d < 256; d <<= 1) {
        unsigned long long xa = 0, xb = 0;
        if (t >= d) { xa = sa[t - d]; xb = sb[t - d]; }
        __syncthreads();
        sa[t] += xa; sb[t] += xb;
        __syncthreads();
    }
    *ta = sa[255]; *tb = sb[255];
    a = sa[t] - a0; b = sb[t] - b0;
    __syncthreads();
}
__global__ __launch_bounds__(256) void k_rows_unpack_sums(const uint32_t *bs32, const uint32_t *us32, uint32_t n, unsigned long long *sums) {
    __shared__ unsigned long long sa[256], sb[256];
    const uint32_t lo = blockIdx.x * 1024 + threadIdx.x * 4;
    unsigned long long a = 0, b = 0, ta, tb;
    for (uint32_t k = 0; k < 4; k++) if (lo + k < n) { a += bs32[lo + k]; b += us32[lo + k]; }
    block_excl_scan2(a, b, sa, sb, &ta, &tb);
    if (threadIdx.x == 0) { sums[2 * blockIdx.x] = ta; sums[2 * blockIdx.x + 1] = tb; }
}
__global__ __launch_bounds__(256) void k_rows_unpack_scan(unsigned long long *sums, uint32_t nblk) {  // exclusive, in place, one workgroup
    __shared__ unsigned long long sa[256], sb[256];
    unsigned long long ca = 0, cb = 0;
    for (uint32_t b0 = 0; b0 < nblk; b0 += 256) {
        const uint32_t i = b0 + threadIdx.x;
        unsigned long long a = i < nblk ? sums[2 * i] : 0, b = i < nblk ? sums[2 * i + 1] : 0, ta, tb;
        block_excl_scan2(a, b, sa, sb, &ta, &tb);
        if (i < nblk) { sums[2 * i] = ca + a; sums[2 * i + 1] = cb + b; }
        ca += ta; cb += tb;
    }
}
__global__ __launch_bounds__(256) void k_rows_unpack_fill(const uint32_t *bs32, const uint32_t *us32, uint32_t n, const unsigned long long *sums,
                                                          uint64_t bo0, uint64_t oo0, uint64_t *bo, uint64_t *bs, uint64_t *oo, uint64_t *us) {
    __shared__ unsigned long long sa[256], sb[256];
    const uint32_t lo = blockIdx.x * 1024 + threadIdx.x * 4;
    uint32_t vb[4] = {0, 0, 0, 0}, vu[4] = {0, 0, 0, 0};
    unsigned long long a = 0, b = 0, ta, tb;
    for (uint32_t k = 0; k < 4; k++) if (lo + k < n) { vb[k] = bs32[lo + k]; vu[k] = us32[lo + k]; a += vb[k]; b += vu[k]; }
    block_excl_scan2(a, b, sa, sb, &ta, &tb);
    unsigned long long pb = bo0 + sums[2 * blockIdx.x] + a, po = oo0 + sums[2 * blockIdx.x + 1] + b;
    for (uint32_t k = 0; k < 4; k++) if (lo + k < n) {
        bo[lo + k] = pb; bs[lo + k] = vb[k]; oo[lo + k] = po; us[lo + k] = vu[k];
        pb += vb[k]; po += vu[k];
    }
}

// verify-only runs: the scratch slot of every row (compressed rows with bytes: their length rounded up to 16; the others take nothing
// and get the position of the next slot), the same three steps per 1,024 rows; sums[2 nblk] = the slots' extent.  A crafted index
// cannot wrap the sums: a row counts for at most VS_ROW_MAX and a group of 1,024 rows for at most VS_GROUP_MAX, both above the
// pool's cap, so such a table comes out with an extent the pool refuses (its offsets are then never used).
constexpr unsigned long long VS_ROW_MAX = (16ull << 30) + 16, VS_GROUP_MAX = 32ull << 30;
__device__ __forceinline__ unsigned long long vs_slot_bytes(const uint8_t *comp, const uint64_t *usize, uint32_t i) {
    if (!comp[i]) return 0ull;
    const unsigned long long u = usize[i];
    return u >= VS_ROW_MAX ? VS_ROW_MAX : (u + 15) & ~15ull;
}
__global__ __launch_bounds__(256) void k_rows_slot_sums(const uint8_t *comp, const uint64_t *usize, uint32_t n, unsigned long long *sums) {
    __shared__ unsigned long long sa[256], sb[256];
    const uint32_t lo = blockIdx.x * 1024 + threadIdx.x * 4;
    unsigned long long a = 0, b = 0, ta, tb;
    for (uint32_t k = 0; k < 4; k++) if (lo + k < n) a += vs_slot_bytes(comp, usize, lo + k);
    block_excl_scan2(a, b, sa, sb, &ta, &tb);
    if (threadIdx.x == 0) { sums[2 * blockIdx.x] = ta < VS_GROUP_MAX ? ta : VS_GROUP_MAX; sums[2 * blockIdx.x + 1] = 0; }
}
__global__ __launch_bounds__(256) void k_rows_slot_fill(const uint8_t *comp, const uint64_t *usize, uint32_t n, unsigned long long *sums, uint32_t nblk, uint64_t *slot_off) {
    __shared__ unsigned long long sa[256], sb[256];
    const uint32_t lo = blockIdx.x * 1024 + threadIdx.x * 4;
    unsigned long long v[4] = {0, 0, 0, 0}, a = 0, b = 0, ta, tb;
    for (uint32_t k = 0; k < 4; k++) if (lo + k < n) { v[k] = vs_slot_bytes(comp, usize, lo + k); a += v[k]; }
    block_excl_scan2(a, b, sa, sb, &ta, &tb);
    unsigned long long at = sums[2 * blockIdx.x] + a;
    for (uint32_t k = 0; k < 4; k++) if (lo + k < n) { slot_off[lo + k] = at; at += v[k]; }
    if (blockIdx.x == nblk - 1 && threadIdx.x == 0) sums[2 * nblk] = sums[2 * blockIdx.x] + (ta < VS_GROUP_MAX ? ta : VS_GROUP_MAX);
}

__global__ void k_iota32(uint32_t *p, uint32_t n) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = i;
}

// rows: the bit column -> one byte per row, and a stored row's length = its blob (the reference hashes and writes the
// blob bytes of a stored row and never looks at the index's uncompressed_size for it, decompress.rs:L143-166)
__global__ void k_rows_fixup(const uint8_t *bitmap, uint64_t row_begin, uint32_t n, uint8_t *comp, uint64_t *usize, const uint64_t *blob_size) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t row = row_begin + i;
    const uint8_t c = bitmap ? (bitmap[row >> 3] >> (row & 7)) & 1 : 1;
    comp[i] = c;
    if (!c) usize[i] = blob_size[i];
}

// ---- the encoder plan of a Round table, built on the device (znippy_rounds_create) ----
// One item per output piece, in round order: an encoded round is ceil(len / 128 KiB) blocks (item.prov = the block's
// provisional slot), a store-path round ceil(len / 64 KiB) pieces (item.prov = the piece's offset inside the round).
struct RoundCount { uint32_t items, small, wide; uint64_t prov; };
__device__ __forceinline__ RoundCount round_count(uint64_t L, uint32_t sk) {
    RoundCount c;
    if (sk) { c.items = (uint32_t)(L ? (L + SKIP_PIECE - 1) / SKIP_PIECE : 1); c.small = 0; c.wide = 0; c.prov = 0; return c; }
    const uint32_t nb = (uint32_t)(L ? (L + BLOCK_BYTES - 1) / BLOCK_BYTES : 1);
    const uint32_t tail = (uint32_t)(L - (uint64_t)(nb - 1) * BLOCK_BYTES), tw = tail > 16 * 1024 ? 1u : 0u;
    c.items = nb; c.wide = nb - 1 + tw; c.small = 1 - tw;
    c.prov = (uint64_t)(nb - 1) * enc_slot_bytes(BLOCK_BYTES) + enc_slot_bytes(tail);
    return c;
}
// Three small kernels: per-workgroup sums of the four per-round counts (1,024 rounds per workgroup), their exclusive scan
// (one workgroup), and the fill — every workgroup scans its own 1,024 rounds again on chip, adds its base and writes its
// rounds' items.  (A first version scanned all rounds in ONE workgroup, every thread a contiguous run: 0.42 ms per 100k
// rounds of strided reads, in front of the table's first encode.)
struct RoundSums { uint32_t items, small, wide, pad; uint64_t prov; };
__device__ __forceinline__ void round_block_scan(uint32_t &ai, uint32_t &as, uint32_t &aw, uint64_t &ap, uint32_t *s_i, uint32_t *s_s, uint32_t *s_w, uint64_t *s_p,
                                                 RoundSums *total) {
    // inclusive scan over the 256 threads of the workgroup (values in / exclusive prefixes out); *total = the workgroup's sums
    const uint32_t t = threadIdx.x;
    const uint32_t vi = ai, vs = as, vw = aw;
    const uint64_t vp = ap;
    s_i[t] = ai; s_s[t] = as; s_w[t] = aw; s_p[t] = ap;
    __syncthreads();
    for (uint32_t d = 1; d < 256; d <<= 1) {
        uint32_t bi = 0, bs = 0, bw = 0; uint64_t bp = 0;
        if (t >= d) { bi = s_i[t - d]; bs = s_s[t - d]; bw = s_w[t - d]; bp = s_p[t - d]; }
        __syncthreads();
        s_i[t] += bi; s_s[t] += bs; s_w[t] += bw; s_p[t] += bp;
        __syncthreads();
    }
    ai = s_i[t] - vi; as = s_s[t] - vs; aw = s_w[t] - vw; ap = s_p[t] - vp;
    if (total) { total->items = s_i[255]; total->small = s_s[255]; total->wide = s_w[255]; total->pad = 0; total->prov = s_p[255]; }
    __syncthreads();
}
__global__ __launch_bounds__(256) void k_rounds_sums(const uint64_t *len, const uint8_t *skip, uint32_t n, RoundSums *sums) {
    __shared__ uint32_t s_i[256], s_s[256], s_w[256];
    __shared__ uint64_t s_p[256];
    const uint32_t lo = blockIdx.x * 1024 + threadIdx.x * 4;
    uint32_t ai = 0, as = 0, aw = 0;
    uint64_t ap = 0;
    for (uint32_t i = lo; i < lo + 4 && i < n; i++) { const RoundCount c = round_count(len[i], skip ? skip[i] : 0); ai += c.items; as += c.small; aw += c.wide; ap += c.prov; }
    RoundSums tot;
    round_block_scan(ai, as, aw, ap, s_i, s_s, s_w, s_p, &tot);
    if (threadIdx.x == 0) sums[blockIdx.x] = tot;
}
__global__ __launch_bounds__(256) void k_rounds_scan(RoundSums *sums, uint32_t nblk) {  // exclusive scan of the workgroup sums, in place
    __shared__ uint32_t s_i[256], s_s[256], s_w[256];
    __shared__ uint64_t s_p[256];
    RoundSums carry{0, 0, 0, 0, 0};
    for (uint32_t b0 = 0; b0 < nblk; b0 += 256) {
        const uint32_t b = b0 + threadIdx.x;
        RoundSums v{0, 0, 0, 0, 0};
        if (b < nblk) v = sums[b];
        uint32_t ai = v.items, as = v.small, aw = v.wide;
        uint64_t ap = v.prov;
        RoundSums tot;
        round_block_scan(ai, as, aw, ap, s_i, s_s, s_w, s_p, &tot);
        if (b < nblk) sums[b] = RoundSums{carry.items + ai, carry.small + as, carry.wide + aw, 0, carry.prov + ap};
        carry.items += tot.items; carry.small += tot.small; carry.wide += tot.wide; carry.prov += tot.prov;
    }
}
__global__ __launch_bounds__(256) void k_rounds_fill(const uint64_t *len, const uint8_t *skip, uint32_t n, const RoundSums *sums, uint32_t *first_item,
                                                      EncItem *items, uint32_t *plen, uint32_t *ord_small, uint32_t *ord_wide) {
    __shared__ uint32_t s_i[256], s_s[256], s_w[256];
    __shared__ uint64_t s_p[256];
    const uint32_t lo = blockIdx.x * 1024 + threadIdx.x * 4;
    RoundCount c[4];
    uint32_t ai = 0, as = 0, aw = 0;
    uint64_t ap = 0;
    for (uint32_t q = 0; q < 4; q++) {
        const uint32_t i = lo + q;
        c[q] = i < n ? round_count(len[i], skip ? skip[i] : 0) : RoundCount{0, 0, 0, 0};
        ai += c[q].items; as += c[q].small; aw += c[q].wide; ap += c[q].prov;
    }
    round_block_scan(ai, as, aw, ap, s_i, s_s, s_w, s_p, nullptr);
    const RoundSums base = sums[blockIdx.x];
    uint32_t at = base.items + ai, so = base.small + as, wo = base.wide + aw;
    uint64_t prov = base.prov + ap;
    for (uint32_t q = 0; q < 4; q++) {
        const uint32_t i = lo + q;
        if (i >= n) break;
        const uint64_t L = len[i];
        first_item[i] = at;
        if (skip && skip[i]) {
            const uint32_t np = c[q].items;
            for (uint32_t k = 0; k < np; k++) {
                const uint64_t o = (uint64_t)k * SKIP_PIECE;
                items[at + k] = EncItem{i, k, np, ITEM_SKIP | (k == 0 ? ITEM_FIRST : 0u), o};
                plen[at + k] = (uint32_t)(L - o < SKIP_PIECE ? L - o : SKIP_PIECE);
            }
            at += np;
            continue;
        }
        const uint32_t nb = c[q].items;
        for (uint32_t k = 0; k < nb; k++) {
            const uint32_t bl = (uint32_t)(L - (uint64_t)k * BLOCK_BYTES < BLOCK_BYTES ? L - (uint64_t)k * BLOCK_BYTES : BLOCK_BYTES);
            if (bl > 16 * 1024) ord_wide[wo++] = at + k; else ord_small[so++] = at + k;
            items[at + k] = EncItem{i, k, nb, k == 0 ? ITEM_FIRST : 0u, prov};
            plen[at + k] = 0;
            prov += enc_slot_bytes(bl);
        }
        at += nb;
    }
}

extern "C" {

int znippy_ctx_create(int device, void *hip_stream, znippy_ctx **out) {
    if (!out) return ZNIPPY_E_INVAL;
    znippy_ctx *ctx = new znippy_ctx();
    ctx->device = device;
    read_switches(ctx);
    if (hipSetDevice(device) != hipSuccess) { delete ctx; return ZNIPPY_E_HIP; }
    if (hip_stream) ctx->stream = (hipStream_t)hip_stream;
    else {
        if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) { delete ctx; return ZNIPPY_E_HIP; }
        ctx->own_stream = true;
    }
    init_fused_tables();
    if (hipStreamCreateWithFlags(&ctx->aux, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&ctx->copy, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->ev_join2, hipEventDisableTiming) != hipSuccess) {
        znippy_ctx_destroy(ctx);
        return ZNIPPY_E_HIP;
    }
    ctx->decode_grid = decode_grid_size(device);
    if (hipMalloc(&ctx->cursor, 64) != hipSuccess) {
        znippy_ctx_destroy(ctx);
        return ZNIPPY_E_NOMEM;
    }
    if (ctx->sw.poison) (void)poison_dev(ctx, ctx->cursor, 64);
    {
        hipDeviceProp_t p;
        int cus = hipGetDeviceProperties(&p, device) == hipSuccess ? p.multiProcessorCount : 256;
        ctx->cus = cus;
        ctx->encode_grid = cus * 8;         // 16 KiB hash table per wave
        ctx->encode_grid_small = cus * 16;  // 4 KiB hash table per wave
    }
    if (!ctx->sw.no_fork_verify) {
        // gfx950: 512 registers per SIMD lane handed out in blocks of 8, 160 KiB of LDS per CU; a workgroup of k_verify is one wave per SIMD.
        // (The role-split kernel's side is what it holds of a CU with all its workgroups resident — two of eight waves and 74 KiB
        // by default: 4 x 120 registers + 32, 148.3 KiB + 192 bytes, five waves per SIMD.  Its registers must stay <= 120 for this.)
        int rr = 0, rw = 0, rl = 0, vr = 0, vl = 0;
        if (roles_footprint(&rr, &rw, &rl) == 0 && verify_footprint(&vr, &vl) == 0)
            ctx->fork_verify = rw * ((rr + 7) / 8 * 8) + (vr + 7) / 8 * 8 <= 512 && rl + vl <= 160 * 1024 && rw + 1 <= 8;
    }
    // Run lanes: the same gate (the verify then runs beside the SUCCESSOR's workgroups, whose footprint is the same), and only on
    // a stream of the context's own: work a caller queues on ITS stream behind a call sees the run's bytes, as the header promises
    if (ctx->fork_verify && ctx->own_stream && !ctx->sw.no_run_lanes) {
        if (hipStreamCreateWithFlags(&ctx->lane, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&ctx->ev_mark, hipEventDisableTiming) != hipSuccess) {
            znippy_ctx_destroy(ctx);
            return ZNIPPY_E_HIP;
        }
        for (auto &pair : ctx->lane_ev)
            for (hipEvent_t &e : pair)
                if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { znippy_ctx_destroy(ctx); return ZNIPPY_E_HIP; }
        ctx->lanes_on = true;
    }
    *out = ctx;
    return ZNIPPY_OK;
}

static void ctx_teardown(znippy_ctx *ctx);
void znippy_ctx_destroy(znippy_ctx *ctx) {
    if (!ctx || ctx->closing) return;
    if (ctx->live_tables) {  // tables outlive the call: they keep the context's memory until the last of them is destroyed
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
        (void)lanes_sync(ctx);
        if (ctx->aux) (void)hipStreamSynchronize(ctx->aux);
        ctx->closing = true;
        return;
    }
    ctx_teardown(ctx);
}
static void table_released(znippy_ctx *ctx) {
    if (--ctx->live_tables == 0 && ctx->closing) ctx_teardown(ctx);
}
static void ctx_teardown(znippy_ctx *ctx) {
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    (void)lanes_sync(ctx);
    if (ctx->aux) (void)hipStreamSynchronize(ctx->aux);
    for (auto &k : ctx->ktimes) { (void)hipEventDestroy(k.t0); (void)hipEventDestroy(k.t1); }
    void *dev[] = {ctx->lit_scratch, ctx->lit_scratch_b, ctx->fz_lit_pool, ctx->fz_seq_pool, ctx->bx_fse_pool, ctx->bx_huf_pool, ctx->rx_pool, ctx->rx_chunk, ctx->rx_cdone, ctx->cursor, ctx->vs_pool, ctx->rr_pool[0], ctx->rr_pool[1],
                   ctx->clk_buf, ctx->shim_in, ctx->shim_out, ctx->enc_prov, ctx->enc_seq, ctx->enc_tabs, ctx->ldm};
    for (void *p : dev) if (p) (void)hipFree(p);
    for (unsigned long long *d : ctx->diag) if (d) (void)hipFree(d);
    if (ctx->aux) { (void)hipStreamSynchronize(ctx->aux); (void)hipStreamDestroy(ctx->aux); }
    if (ctx->copy) { (void)hipStreamSynchronize(ctx->copy); (void)hipStreamDestroy(ctx->copy); }
    if (ctx->lane) (void)hipStreamDestroy(ctx->lane);
    if (ctx->ev_mark) (void)hipEventDestroy(ctx->ev_mark);
    for (auto &pair : ctx->lane_ev)
        for (hipEvent_t e : pair) if (e) (void)hipEventDestroy(e);
    for (auto &e : ctx->pinned_pool) (void)hipHostFree(e.second);
    for (auto &e : ctx->dev_pool) (void)hipFree(e.second);
    for (hipEvent_t e : ctx->event_pool) (void)hipEventDestroy(e);
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    if (ctx->ev_join) (void)hipEventDestroy(ctx->ev_join);
    if (ctx->ev_join2) (void)hipEventDestroy(ctx->ev_join2);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

const char *znippy_last_error(const znippy_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int znippy_ctx_sync(znippy_ctx *ctx) {
    if (!ctx_enter(ctx)) return ZNIPPY_E_INVAL;
    if (!ctx) return ZNIPPY_E_INVAL;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, lanes_sync(ctx));  // a lean run's kernel may be queued there (lane_begin)
    if (ctx->aux) HIPCHK(ctx, hipStreamSynchronize(ctx->aux));  // a run's verify and result copy may be queued there (run_verify)
    if (ctx->copy) HIPCHK(ctx, hipStreamSynchronize(ctx->copy));
    return ZNIPPY_OK;
}

int znippy_last_kernel_times(znippy_ctx *ctx, const char **names, float *ms, int cap) {
    if (!ctx_enter(ctx, ENTER_HOST)) return ZNIPPY_E_INVAL;
    if (!ctx) return 0;
    int n = std::min(cap, ctx->n_ktimes);
    for (int i = 0; i < n; i++) {
        names[i] = ctx->ktimes[i].name;
        ms[i] = 0.f;
        (void)hipEventElapsedTime(&ms[i], ctx->ktimes[i].t0, ctx->ktimes[i].t1);
    }
    return n;
}

int znippy_ctx_run_lane_stats(znippy_ctx *ctx, uint64_t out[4]) {
    if (!ctx || ctx->closing || !out) return ZNIPPY_E_INVAL;  // (queues nothing: the lanes stay as they are)
    memcpy(out, ctx->lane_stats, 4 * sizeof(uint64_t));
    return ZNIPPY_OK;
}
int znippy_ctx_run_lane_older_waits(znippy_ctx *ctx, uint64_t *out) {
    if (!ctx || ctx->closing || !out) return ZNIPPY_E_INVAL;
    *out = ctx->lane_stats[4];
    return ZNIPPY_OK;
}

int znippy_rows_foreign_stats(znippy_ctx *ctx, znippy_rows *r, uint64_t stats[8]) {
    if (!ctx_enter(ctx)) return ZNIPPY_E_INVAL;
    if (!ctx || !r || r->ctx != ctx || !stats) return ZNIPPY_E_INVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    // the pool counters of the path that ran for this table: the batch path's or the round-2 two-phase path's
    HIPCHK(ctx, hipMemcpy(stats, r->ctl + (r->shape.bx_slots ? CTL_BX_POOL : CTL_FZ_POOL).at, 64, hipMemcpyDeviceToHost));
    return ZNIPPY_OK;
}

int znippy_rows_checksum_stats(znippy_ctx *ctx, znippy_rows *r, uint64_t stats[4]) {
    if (!ctx_enter(ctx)) return ZNIPPY_E_INVAL;
    if (!ctx || !r || r->ctx != ctx || !stats) return ZNIPPY_E_INVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    static_assert(CTL_BX_XXH.bytes == 4 * sizeof(uint64_t), "checksum_stats");
    HIPCHK(ctx, hipMemcpy(stats, r->ctl + CTL_BX_XXH.at, CTL_BX_XXH.bytes, hipMemcpyDeviceToHost));
    stats[3] = 0;
    return ZNIPPY_OK;
}

int znippy_ctx_set_batch_checksums(znippy_ctx *ctx, int on) {
    if (!ctx_enter(ctx, ENTER_HOST)) return ZNIPPY_E_INVAL;
    if (!ctx || (on != 0 && on != 1)) return ZNIPPY_E_INVAL;
    ctx->batch_checksums = on;
    return ZNIPPY_OK;
}

int znippy_ctx_batch_checksums(const znippy_ctx *ctx) { return ctx && !ctx->closing ? ctx->batch_checksums : ZNIPPY_E_INVAL; }

int znippy_ctx_set_level(znippy_ctx *ctx, int level) {
    if (!ctx_enter(ctx, ENTER_HOST)) return ZNIPPY_E_INVAL;
    if (!ctx || level < 1 || level > 22) return ZNIPPY_E_INVAL;
    ctx->level = level;
    return ZNIPPY_OK;
}

int znippy_ctx_level(const znippy_ctx *ctx) { return ctx ? ctx->level : ZNIPPY_E_INVAL; }

int znippy_ctx_set_window_log(znippy_ctx *ctx, int window_log) {
    if (!ctx_enter(ctx, ENTER_HOST)) return ZNIPPY_E_INVAL;
    if (!ctx || (window_log != 0 && (window_log < WINDOW_LOG_MIN || window_log > WINDOW_LOG_MAX))) return ZNIPPY_E_INVAL;
    ctx->window_log = window_log;
    return ZNIPPY_OK;
}

int znippy_ctx_window_log(const znippy_ctx *ctx) { return ctx && !ctx->closing ? ctx->window_log : ZNIPPY_E_INVAL; }

int znippy_ctx_set_gunzip_cut(znippy_ctx *ctx, uint64_t cut_bytes) {
    if (!ctx_enter(ctx, ENTER_HOST)) return ZNIPPY_E_INVAL;
    if (!ctx || !gzcut::cut_valid(cut_bytes)) return ZNIPPY_E_INVAL;
    ctx->gz_cut = cut_bytes;
    return ZNIPPY_OK;
}

uint64_t znippy_ctx_gunzip_cut(const znippy_ctx *ctx) { return ctx && !ctx->closing ? ctx->gz_cut : 0; }

int znippy_ctx_gunzip_cut_stats(znippy_ctx *ctx, uint64_t out[8]) {
    if (!ctx_enter(ctx, ENTER_HOST)) return ZNIPPY_E_INVAL;
    if (!ctx || !out) return ZNIPPY_E_INVAL;
    memcpy(out, ctx->gz_cut_stats, sizeof ctx->gz_cut_stats);
    return ZNIPPY_OK;
}

int znippy_ctx_set_kernel_timing(znippy_ctx *ctx, int level) {
    if (!ctx_enter(ctx, ENTER_HOST)) return ZNIPPY_E_INVAL;
    if (!ctx || level < 0 || level > 2) return ZNIPPY_E_INVAL;
    ctx->sw.ktime = level;
    return ZNIPPY_OK;
}

int znippy_measure_blake3_pass_ns(znippy_ctx *ctx, float *ns_per_pass_per_simd, float *shader_ghz) {
    if (!ctx_enter(ctx)) return ZNIPPY_E_INVAL;
    if (!ctx || !ns_per_pass_per_simd) return ZNIPPY_E_INVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return measure_b3_pass_ns(ctx->cus, ctx->stream, ns_per_pass_per_simd, shader_ghz);
}

// Shader clock a read-side kernel held during the last run with ZNIPPY_DBG bit 32768 set: one wave's life in shader
// cycles / in 100 MHz ticks (MI355X_MICROARCH.md, DVFS give-back (6)).  0 if nothing was recorded.
int znippy_last_shader_ghz(znippy_ctx *ctx, float *ghz) {
    if (!ctx_enter(ctx)) return ZNIPPY_E_INVAL;
    if (!ctx || !ghz) return ZNIPPY_E_INVAL;
    *ghz = 0.f;
    if (!ctx->clk_buf) return ZNIPPY_OK;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    unsigned long long h[2] = {0, 0};
    HIPCHK(ctx, hipMemcpy(h, ctx->clk_buf, 16, hipMemcpyDeviceToHost));
    if (h[1]) *ghz = (float)((double)h[0] / (double)h[1] * 0.1);
    return ZNIPPY_OK;
}

// The role-split read kernel's geometry and what decides whether a run's verify is forked, and — from a context created with
// ZNIPPY_DBG bit 32768 — the wait counters its waves left in the last run (fused_small.hip: roles_clk_add).
int znippy_roles_wait_stats(znippy_ctx *ctx, uint32_t geometry[8], uint64_t *waves, uint64_t cap_words, uint64_t *n_words) {
    if (!ctx_enter(ctx)) return ZNIPPY_E_INVAL;
    if (!ctx || !geometry || !n_words || (cap_words && !waves)) return ZNIPPY_E_INVAL;
    int rr = 0, rw = 0, rl = 0;
    roles_geometry(geometry);
    if (roles_footprint(&rr, &rw, &rl) != 0) return ZNIPPY_E_HIP;
    geometry[4] = (uint32_t)rr; geometry[5] = (uint32_t)rl; geometry[6] = ctx->fork_verify; geometry[7] = ctx->lanes_on;
    *n_words = 0;
    if (!ctx->clk_buf) return ZNIPPY_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, lanes_sync(ctx));
    const uint64_t have = roles_clk_bytes(ctx->cus) / 8 - 8;
    *n_words = have < cap_words ? have : cap_words;
    if (*n_words) HIPCHK(ctx, hipMemcpy(waves, ctx->clk_buf + 8, *n_words * 8, hipMemcpyDeviceToHost));
    return ZNIPPY_OK;
}

// ---- frame header (host) ------------------------------------------------------------------------
// Leading skippable frames (RFC 8878 3.1.2) carry no content: the single-chunk shims step over them — the size
// query and the decoder both start at the first Zstandard frame.  -1: a skippable frame runs past the input.
static ptrdiff_t skippable_prefix(const uint8_t *p, size_t n) {
    size_t at = 0;
    while (n - at >= 8) {
        uint32_t magic, sz;
        memcpy(&magic, p + at, 4);
        if ((magic & 0xFFFFFFF0u) != 0x184D2A50u) break;
        memcpy(&sz, p + at + 4, 4);
        if ((uint64_t)8 + sz > n - at) return -1;
        at += 8 + (size_t)sz;
    }
    return (ptrdiff_t)at;
}

int znippy_get_decompressed_size(const void *frame, size_t n, uint64_t *out_size) {
    const uint8_t *p = (const uint8_t *)frame;
    if (!p || !out_size) return ZNIPPY_E_INVAL;
    {
        const ptrdiff_t skip = skippable_prefix(p, n);
        if (skip < 0) return ZNIPPY_E_CORRUPT;
        p += skip;
        n -= (size_t)skip;
    }
    if (n < 5) return ZNIPPY_E_CORRUPT;
    uint32_t magic;
    memcpy(&magic, p, 4);
    if (magic != 0xFD2FB528u) return ZNIPPY_E_CORRUPT;
    uint32_t fhd = p[4], fcs_flag = fhd >> 6, single = (fhd >> 5) & 1, did_flag = fhd & 3;
    if (fhd & 8) return ZNIPPY_E_CORRUPT;
    uint32_t fcs_bytes = fcs_flag == 0 ? single : (1u << fcs_flag);
    uint32_t did_bytes = did_flag == 3 ? 4 : did_flag;
    size_t pos = 5 + (single ? 0 : 1) + did_bytes;
    if (n < pos + fcs_bytes) return ZNIPPY_E_CORRUPT;
    if (!fcs_bytes) return ZNIPPY_E_UNSUPPORTED;
    uint64_t fcs = 0;
    for (uint32_t i = 0; i < fcs_bytes; i++) fcs |= (uint64_t)p[pos + i] << (8 * i);
    if (fcs_bytes == 2) fcs += 256;
    *out_size = fcs;
    return ZNIPPY_OK;
}

// ---- rows ---------------------------------------------------------------------------------------

void znippy_rows_destroy(znippy_rows *r) {
    if (!r) return;
    (void)hipSetDevice(r->ctx->device);
    void *ptrs[] = {r->blob_off, r->blob_size, r->usize, r->out_off, r->compressed, r->checksum,
                    r->ctl_m[0], r->ctl_m[1], r->digests_m[0], r->digests_m[1], r->corrupt_m[0], r->corrupt_m[1], r->list_a, r->pending,
                    r->cand_row, r->cand_base, r->cand_nblocks, r->fz_base, r->fz_cap, r->fz_it_cand, r->fz_nb, r->fz_work, r->fz_items, r->item_row, r->item_k, r->item_src, r->row_flag, r->pending2,
                    r->bt_tile, r->bt_item, r->tile_done, r->todo, r->status_init, r->slow_list,
                    r->bx_cand_row, r->bx_cand_base, r->bx_cand_nb, r->bx_huf_list, r->bx_seq_list, r->bx_items, r->bx_prep, r->d_bitmap, r->bx_sort_tmp,
                    r->rx_base, r->rx_fail, r->rx_blk, r->rx_list, r->bx_cand_ck, r->d_pack, r->d_pack_sums, r->all_rows, r->vs_off, r->tree_dev};
    // (the pool hands these buffers to the next table, whose work is ordered on the main stream: what this table still has on
    // the auxiliary stream — a forked verify — is joined into it first)
    // (... and its runs on the run lane: the lanes are closed — no later run is compared with, or waits for an event of, this table —
    // and waited for)
    lanes_close(r->ctx);
    if (r->lane_used) (void)lanes_sync(r->ctx);
    if (r->aux_used && hipEventRecord(r->ctx->ev_join, r->ctx->aux) == hipSuccess) (void)hipStreamWaitEvent(r->ctx->stream, r->ctx->ev_join, 0);
    for (void *p : ptrs)
        tfree(r->ctx, p);
    if (r->h_counters) {
        (void)hipStreamSynchronize(r->ctx->stream);  // a queued run may still write into the slot
        pinned_give(r->ctx, r->h_counters, r->h_counters_cap);
    }
    if (r->h_pack) {
        (void)hipStreamSynchronize(r->ctx->stream);  // (the copy out of it is stream-ordered)
        pinned_give(r->ctx, r->h_pack, r->h_pack_cap);
    }
    for (hipEvent_t e : r->ev_done) event_give(r->ctx, e);
    for (hipEvent_t e : r->ev_main) event_give(r->ctx, e);
    free_plan(r->ctx, r->plan);
    znippy_ctx *const c = r->ctx;
    delete r;
    table_released(c);
}

// the columns as they are (the device derives the byte-per-row flags and the stored rows' lengths), then the checksums
static int rows_columns_h2d(znippy_ctx *ctx, znippy_rows *r, const RowCols &c, const uint8_t *checksum, TDbg &td) {
    const uint32_t n = (uint32_t)(c.row_end - c.row_begin);
    int rc = ZNIPPY_OK;
    const uint64_t bm0 = c.row_begin >> 3, bm1 = (c.row_end + 7) >> 3;  // (d_bitmap is kept until the table goes: k_rows_fixup reads it on the stream, uploads are not stream-ordered)
    // A table written front to back is its two size columns (zn_rows_pack32): 8 bytes per row go to the device, from
    // page-locked memory, and three small kernels make the four 64-bit columns there.  (The four pageable copies of 0.8 MB
    // each were 0.18 of the 0.36 ms a table of 100k rows took to build.)
    bool packed = false;
    if (n >= 64 && !ctx->sw.no_pack) {
        r->h_pack = (uint32_t *)pinned_take(ctx, 8 * (size_t)n, &r->h_pack_cap);
        if (r->h_pack && zn_rows_pack32(c.bo, c.bs, c.oo, c.us, n, r->h_pack)) {
            const uint32_t nblk = (n + 1023) / 1024;
            if (tmalloc(ctx, &r->d_pack, 8 * (size_t)n) != hipSuccess || tmalloc(ctx, &r->d_pack_sums, 16 * (size_t)nblk) != hipSuccess ||
                tmalloc(ctx, &r->blob_off, 8 * (size_t)n) != hipSuccess || tmalloc(ctx, &r->blob_size, 8 * (size_t)n) != hipSuccess ||
                tmalloc(ctx, &r->usize, 8 * (size_t)n) != hipSuccess || tmalloc(ctx, &r->out_off, 8 * (size_t)n) != hipSuccess ||
                hipMemcpyAsync(r->d_pack, r->h_pack, 8 * (size_t)n, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
                return ZNIPPY_E_NOMEM;
            hipLaunchKernelGGL(k_rows_unpack_sums, dim3(nblk), dim3(256), 0, ctx->stream, r->d_pack, r->d_pack + n, n, r->d_pack_sums);
            hipLaunchKernelGGL(k_rows_unpack_scan, dim3(1), dim3(256), 0, ctx->stream, r->d_pack_sums, nblk);
            hipLaunchKernelGGL(k_rows_unpack_fill, dim3(nblk), dim3(256), 0, ctx->stream, r->d_pack, r->d_pack + n, n, r->d_pack_sums, c.bo[0], c.oo[0],
                               r->blob_off, r->blob_size, r->out_off, r->usize);
            packed = true;
        }
    }
    if ((!packed && ((rc = dev_upload(ctx, &r->blob_off, c.bo, n)) || (rc = dev_upload(ctx, &r->blob_size, c.bs, n)) ||
                     (rc = dev_upload(ctx, &r->usize, c.us, n)) || (rc = dev_upload(ctx, &r->out_off, c.oo, n)))) ||
        (c.bitmap && (rc = dev_upload(ctx, &r->d_bitmap, c.bitmap + bm0, (size_t)(bm1 - bm0)))) ||
        tmalloc(ctx, &r->compressed, std::max<size_t>(n, 16)) != hipSuccess)
        return rc ? rc : ZNIPPY_E_NOMEM;
    if (n) hipLaunchKernelGGL(k_rows_fixup, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, r->d_bitmap, c.row_begin - 8 * bm0, n, r->compressed, r->usize, r->blob_size);
    td.mark("columns_h2d");
    if (checksum && (rc = dev_upload(ctx, &r->checksum, checksum + 32 * c.row_begin, (size_t)32 * n))) return rc;
    td.mark("checksum_h2d");
    return ZNIPPY_OK;
}

// what the block-item path, the batch path and the serial decoder tell each other about a row, the serial decoder's list,
// and the batch / resolve paths' per-table buffers (capacities: rows_classify)
static int rows_batch_buffers(znippy_ctx *ctx, znippy_rows *r) {
    const RowsShape &s = r->shape;
    if (tmalloc(ctx, &r->row_flag, std::max<size_t>(4 * (size_t)s.n, 16)) != hipSuccess ||
        tmalloc(ctx, &r->pending2, std::max<size_t>(4 * (size_t)s.n_compressed, 16)) != hipSuccess)
        return ZNIPPY_E_NOMEM;
    if (!s.bx_slots) return ZNIPPY_OK;
    const size_t cap = s.bx_item_cap;
    if (tmalloc(ctx, &r->bx_cand_row, 4 * (size_t)s.bx_slots) != hipSuccess || tmalloc(ctx, &r->bx_cand_base, 4 * (size_t)s.bx_slots) != hipSuccess ||
        tmalloc(ctx, &r->bx_cand_nb, 4 * (size_t)s.bx_slots) != hipSuccess || tmalloc(ctx, &r->bx_huf_list, 4 * cap) != hipSuccess ||
        tmalloc(ctx, &r->bx_seq_list, 4 * 4 * cap) != hipSuccess || tmalloc(ctx, &r->bx_sort_tmp, 5 * 4 * cap) != hipSuccess || tmalloc(ctx, &r->bx_items, sizeof(zn::FzItem) * cap) != hipSuccess ||
        tmalloc(ctx, &r->bx_prep, sizeof(zn::BxPrep) * cap) != hipSuccess ||
        (s.rx_frames &&
         (tmalloc(ctx, &r->rx_base, 4 * (size_t)s.bx_slots) != hipSuccess || tmalloc(ctx, &r->rx_fail, 4 * (size_t)s.bx_slots) != hipSuccess ||
          tmalloc(ctx, &r->rx_blk, 16 * cap) != hipSuccess || tmalloc(ctx, &r->rx_list, 4 * cap) != hipSuccess)))
        return ZNIPPY_E_NOMEM;
    return ZNIPPY_OK;
}
// block items: the candidates, their items, and the round-2 two-phase path's item slots
static int rows_item_buffers(znippy_ctx *ctx, znippy_rows *r, const RowClasses &k) {
    const RowsShape &s = r->shape;
    int rc;
    if ((rc = dev_upload(ctx, &r->cand_row, k.cand_row.data(), k.cand_row.size())) ||
        (rc = dev_upload(ctx, &r->cand_base, k.cand_base.data(), k.cand_base.size())) ||
        (rc = dev_upload(ctx, &r->cand_nblocks, k.cand_nb.data(), k.cand_nb.size())) ||
        (rc = dev_upload(ctx, &r->item_row, k.item_row.data(), k.item_row.size())) ||
        (rc = dev_upload(ctx, &r->item_k, k.item_k.data(), k.item_k.size())))
        return rc;
    if (tmalloc(ctx, &r->item_src, 4 * (size_t)s.n_items) != hipSuccess) return ZNIPPY_E_NOMEM;
    if (!s.fz_total) return ZNIPPY_OK;
    if ((rc = dev_upload(ctx, &r->fz_base, k.fz_base.data(), k.fz_base.size())) ||
        (rc = dev_upload(ctx, &r->fz_cap, k.fz_cap.data(), k.fz_cap.size())) ||
        (rc = dev_upload(ctx, &r->fz_it_cand, k.fz_it_cand.data(), k.fz_it_cand.size())))
        return rc;
    if (tmalloc(ctx, &r->fz_nb, 4 * (size_t)s.n_cand) != hipSuccess || tmalloc(ctx, &r->fz_work, 4 * (size_t)s.fz_total) != hipSuccess ||
        tmalloc(ctx, &r->fz_items, sizeof(zn::FzItem) * (size_t)s.fz_total) != hipSuccess)
        return ZNIPPY_E_NOMEM;
    return ZNIPPY_OK;
}
// fused block kernel: the big-slice tiles of the candidate rows and the item each belongs to, its done flags, what it leaves
static int rows_fused_block_buffers(znippy_ctx *ctx, znippy_rows *r, const RowClasses &k) {
    int rc;
    if ((rc = dev_upload(ctx, &r->bt_tile, k.bt_tile.data(), k.bt_tile.size())) || (rc = dev_upload(ctx, &r->bt_item, k.bt_item.data(), k.bt_item.size()))) return rc;
    size_t items_at;
    r->done_bytes = rows_done_bytes(r->shape, &items_at);
    if (tmalloc(ctx, &r->tile_done, r->done_bytes) != hipSuccess ||
        tmalloc(ctx, &r->todo, std::max<size_t>(4 * (size_t)r->shape.n_items, 16)) != hipSuccess)
        return ZNIPPY_E_NOMEM;
    r->item_done = r->tile_done + items_at;
    return ZNIPPY_OK;
}

int znippy_rows_create(znippy_ctx *ctx, const uint64_t *blob_offset, const uint64_t *blob_size,
                       const uint8_t *compressed_bitmap, const uint64_t *uncompressed_size,
                       const uint64_t *out_offset, const uint8_t *checksum, uint64_t row_begin,
                       uint64_t row_end, znippy_rows **out) {
    if (!ctx_enter(ctx)) return ZNIPPY_E_INVAL;
    if (!ctx || !out || row_end < row_begin || !blob_offset || !blob_size || !uncompressed_size)
        return ZNIPPY_E_INVAL;
    if (row_end - row_begin >= 0xFFFFFFF0ull) return ZNIPPY_E_INVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    TDbg td(ctx->sw.tdbg, "rows_create");
    std::unique_ptr<znippy_rows, void (*)(znippy_rows *)> guard(new znippy_rows(), znippy_rows_destroy);  // every failure below: return
    znippy_rows *const r = guard.get();
    r->ctx = ctx;
    ctx->live_tables++;
    r->row_begin = row_begin;
    const uint32_t n = (uint32_t)(row_end - row_begin);
    const bool allc = rows_all_compressed(compressed_bitmap, row_begin, row_end);
    // a table without output offsets can only be verified (znippy_verify_rows): its output column is a packed layout of its own, so that
    // everything below that looks at the column finds a consistent one
    std::vector<uint64_t> own_oo;
    if (!out_offset) {
        r->no_out = true;
        own_oo.resize(n);
        uint64_t at = 0;
        for (uint32_t i = 0; i < n; i++) { own_oo[i] = at; at += uncompressed_size[row_begin + i]; }
    }
    const RowCols c{blob_offset + row_begin, blob_size + row_begin, uncompressed_size + row_begin, out_offset ? out_offset + row_begin : own_oo.data(), compressed_bitmap, row_begin, row_end, allc};
    int rc = rows_columns_h2d(ctx, r, c, checksum, td);
    if (rc) return rc;
    r->corrupt_cap = std::max<uint32_t>(n, 1);
    r->ctl_bytes = CTL_HEAD + std::max<size_t>(4 * (size_t)n, 16);
    for (int s = 0; s < 2; s++)
        if (tmalloc(ctx, &r->ctl_m[s], r->ctl_bytes) != hipSuccess ||
            tmalloc(ctx, &r->digests_m[s], std::max<size_t>(32 * (size_t)n, 32)) != hipSuccess ||
            tmalloc(ctx, &r->corrupt_m[s], 8 * (size_t)r->corrupt_cap) != hipSuccess ||
            !(r->ev_done[s] = event_take(ctx)) || !(r->ev_main[s] = event_take(ctx)))
            return ZNIPPY_E_NOMEM;
    if (!(r->h_counters = (uint64_t *)pinned_take(ctx, 256, &r->h_counters_cap))) return ZNIPPY_E_NOMEM;
    r->select(0);
    td.mark("allocs");
    PlanBuf p;
    // a stored row IS its blob (see k_rows_fixup): its effective length is blob_size.  (allc and the column pointers by value: the pass over
    // 100k rows keeps them in registers, which it cannot with members of `c`, whose address has left this function)
    build_plan([=, us = c.us, bs = c.bs, &c](uint32_t i) -> uint64_t { return (allc || c.comp(i)) ? us[i] : bs[i]; }, n, p);
    td.mark("plan");
    if ((rc = upload_plan(ctx, p, r->plan))) return rc;
    td.mark("plan_h2d");
    RowsShape &s = r->shape;
    RowClasses k;
    rows_classify(c, ctx->sw, p, s, k);
    if (s.n_small_tiles && tmalloc(ctx, &r->slow_list, 4 * (size_t)s.n_tiles) != hipSuccess) return ZNIPPY_E_NOMEM;
    td.mark("big_rows");
    if (s.n_compressed && (rc = rows_batch_buffers(ctx, r))) return rc;
    if (s.n_cand && (rc = rows_item_buffers(ctx, r, k))) return rc;
    if (s.n_bt && (rc = rows_fused_block_buffers(ctx, r, k))) return rc;
    if ((rc = dev_upload(ctx, &r->list_a, k.la.data(), k.la.size()))) return rc;
    if (tmalloc(ctx, &r->pending, std::max<size_t>(4 * (size_t)n, 16)) != hipSuccess) return ZNIPPY_E_NOMEM;
    td.mark("rest");
    *out = guard.release();
    return ZNIPPY_OK;
}

int znippy_rows_set_blob_cap(znippy_rows *r, uint64_t blob_cap) {
    if (!r) return ZNIPPY_E_INVAL;
    r->blob_cap = blob_cap;
    return ZNIPPY_OK;
}

// Every row's source range against the declared blob region and its output range against out_cap, overflow-safe,
// once per distinct triple.  Bad rows (normally none) get their status from the host.
// (verify-only runs: the output side is the table's own slots in the scratch, which fit by construction — only the blob side is looked at)
static int rows_validate(znippy_ctx *ctx, znippy_rows *r, uint64_t blob_base, uint64_t out_cap, bool verify) {
    if (verify) out_cap = ~0ull;
    if (r->val_done && r->val_verify == verify && r->val_base == blob_base && r->val_bcap == r->blob_cap && r->val_ocap == out_cap) return ZNIPPY_OK;
    std::vector<int32_t> init;
    const bool fits = rows_fit(r->shape, blob_base, r->blob_cap, out_cap, verify);
    if (!fits && r->h_blob_off.empty() && r->shape.n) {  // the columns, for the per-row verdicts (the device copies hold the effective lengths)
        r->h_blob_off.resize(r->shape.n); r->h_blob_size.resize(r->shape.n); r->h_len.resize(r->shape.n);
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        HIPCHK(ctx, hipMemcpy(r->h_blob_off.data(), r->blob_off, 8 * (size_t)r->shape.n, hipMemcpyDeviceToHost));
        HIPCHK(ctx, hipMemcpy(r->h_blob_size.data(), r->blob_size, 8 * (size_t)r->shape.n, hipMemcpyDeviceToHost));
        HIPCHK(ctx, hipMemcpy(r->h_len.data(), r->usize, 8 * (size_t)r->shape.n, hipMemcpyDeviceToHost));
    }
    if (!fits && !verify && r->h_out_off.empty() && r->shape.n) {
        r->h_out_off.resize(r->shape.n);
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        HIPCHK(ctx, hipMemcpy(r->h_out_off.data(), r->out_off, 8 * (size_t)r->shape.n, hipMemcpyDeviceToHost));
    }
    const uint32_t bad = fits ? 0 : rows_verdicts(r->h_blob_off.data(), r->h_blob_size.data(), r->h_len.data(), r->h_out_off.data(), r->shape.n, blob_base, r->blob_cap, out_cap, verify, init);
    if (bad) {
        // image of the whole control block: zero head + the preset status column
        if (!r->status_init) {
            if (tmalloc(ctx, &r->status_init, r->ctl_bytes) != hipSuccess) return ZNIPPY_E_NOMEM;
            HIPCHK(ctx, hipMemset(r->status_init, 0, r->ctl_bytes));
        }
        HIPCHK(ctx, hipMemcpy(r->status_init + CTL_HEAD, init.data(), 4 * (size_t)r->shape.n, hipMemcpyHostToDevice));
    }
    r->hints.n_bad = bad;
    r->val_base = blob_base; r->val_bcap = r->blob_cap; r->val_ocap = out_cap;
    r->val_done = true; r->val_verify = verify;
    return ZNIPPY_OK;
}

// The table's slots in the verify scratch, once (the first verify-only run, or the hook): built on the device from the columns the kernels
// read — a stored row's length there is its blob, and it gets no slot — and the extent comes back for the pool.
static int rows_verify_slots(znippy_ctx *ctx, znippy_rows *r) {
    if (r->vs_built) return ZNIPPY_OK;
    if (r->shape.n && r->shape.n_compressed) {
        const uint32_t nblk = (r->shape.n + 1023) / 1024;
        unsigned long long *sums = nullptr;
        if (tmalloc(ctx, &r->vs_off, 8 * (size_t)r->shape.n) != hipSuccess) return ZNIPPY_E_NOMEM;
        if (tmalloc(ctx, &sums, 16 * ((size_t)nblk + 1)) != hipSuccess) return ZNIPPY_E_NOMEM;
        hipLaunchKernelGGL(k_rows_slot_sums, dim3(nblk), dim3(256), 0, ctx->stream, r->compressed, r->usize, r->shape.n, sums);
        hipLaunchKernelGGL(k_rows_unpack_scan, dim3(1), dim3(256), 0, ctx->stream, sums, nblk);
        hipLaunchKernelGGL(k_rows_slot_fill, dim3(nblk), dim3(256), 0, ctx->stream, r->compressed, r->usize, r->shape.n, sums, nblk, r->vs_off);
        unsigned long long total = 0;
        const hipError_t e1 = hipStreamSynchronize(ctx->stream), e2 = hipMemcpy(&total, sums + 2 * (size_t)nblk, 8, hipMemcpyDeviceToHost);
        tfree(ctx, sums);
        HIPCHK(ctx, e1);
        HIPCHK(ctx, e2);
        r->vs_bytes = total;
    } else if (r->shape.n) {  // no compressed row: no slot, no scratch — the column exists (every row: position 0) because the kernels load it
        if (tmalloc(ctx, &r->vs_off, 8 * (size_t)r->shape.n) != hipSuccess) return ZNIPPY_E_NOMEM;
        HIPCHK(ctx, hipMemsetAsync(r->vs_off, 0, 8 * (size_t)r->shape.n, ctx->stream));
    }
    r->vs_built = true;
    return ZNIPPY_OK;
}

// ---- one run of a row table: the plan (host/rows_plan.h: rows_plan), then the stages in the order rows_launch queues them ----------
// the context and the table's optional buffers as this run finds them; nothing here or in the plan calls HIP
static RunEnv rows_run_env(const znippy_ctx *ctx, const znippy_rows *r, const void *d_out) {
    return RunEnv{ctx->fz_lit_pool != nullptr, ctx->fz_seq_pool != nullptr, ctx->bx_fse_pool != nullptr, ctx->bx_huf_pool != nullptr, ctx->rx_pool != nullptr, r->rx_base != nullptr,
                  ctx->rx_cap, ctx->cus, ctx->decode_grid, ctx->gen_share, ctx->batch_checksums && r->bx_cand_ck, ctx->fork_verify, ((uintptr_t)d_out & 15) != 0, &ctx->sw};
}

static HashArgs rows_hash_args(const znippy_ctx *ctx, const znippy_rows *r, const RunPlan &p, const RowsRun &run) {
    HashArgs h{};
    h.tiles = r->plan.tiles; h.n_tiles = r->plan.n_tiles;
    h.len = r->usize;
    h.srcA = (const uint8_t *)run.d_blobs; h.offA = r->blob_off; h.baseA = run.blob_base;
    h.srcB = (uint8_t *)run.d_out; h.offB = run.verify ? r->vs_off : r->out_off;
    h.sel = r->compressed; h.status = r->status; h.pending_count = r->hand(H_FUSED);
    // (verify-only: stored rows are hashed where they lie by the hash-only kernel, nothing is copied.  The store path's staged loads with
    // the stores left out were measured in its place: equal on big slices, 8 % slower on C5 and on tables of small stored rows.)
    h.copy_to_B = run.verify ? 0 : 1;
    h.store_tiles = ctx->sw.store_g;
    h.misaligned_dst = p.misaligned_dst;
    h.digests = r->digests; h.tile_cv = r->plan.tile_cv;
    return h;
}
static BlockScanArgs rows_scan_args(const znippy_rows *r, const RowsRun &run) {
    BlockScanArgs b{};
    b.cand_row = r->cand_row; b.cand_base = r->cand_base; b.cand_nblocks = r->cand_nblocks; b.n_cand = r->shape.n_cand;
    fill_row_args(b, r, run);
    b.item_src = r->item_src; b.row_flag = r->row_flag;
    b.pending = r->pending2; b.pending_count = r->hand(H_SERIAL);  // its own hand-over list
    return b;
}
// the serial decoder over the host's list and what the fused kernels handed over; decode_rest turns it to what everything left
static DecodeArgs rows_decode_args(znippy_ctx *ctx, const znippy_rows *r, const RowsRun &run) {
    DecodeArgs a{};
    fill_row_args(a, r, run);
    a.list_a = r->list_a; a.n_list_a = r->shape.n_list_a;
    a.pending = r->pending; a.pending_count = r->hand(H_FUSED);
    a.compressed = r->compressed;
    a.n_rows = r->shape.n; a.cursor = r->cur(CUR_GENERAL);
    a.lit_scratch = ctx->lit_scratch;
    if (ctx->sw.ddbg)  // diagnostic: phase shares of the previous general-decoder launch
        a.dbg = diag_cycle<8>(ctx, znippy_ctx::DIAG_GENERAL, ctx->stream, nullptr, [](const unsigned long long *h) {
            if (h[0]) fprintf(stderr, "[znippy ddbg] general decoder frames=%llu  kcycles per frame: headers+tree=%.1f huffman-table=%.1f literal-streams=%.1f seq-tables=%.1f first-batch=%.1f decode+execute=%.1f tail=%.1f\n", h[0],
                              h[6] / 1e3 / h[0], h[7] / 1e3 / h[0], h[1] / 1e3 / h[0], h[2] / 1e3 / h[0], h[3] / 1e3 / h[0], h[4] / 1e3 / h[0], h[5] / 1e3 / h[0]);
        });
    return a;
}
static void decode_rest(znippy_ctx *ctx, const znippy_rows *r, const RunPlan &p, DecodeArgs a) {  // what every path left: pending2
    a.list_a = nullptr; a.n_list_a = 0;
    a.pending = r->pending2; a.pending_count = r->hand(H_SERIAL);
    a.cursor = r->cur(CUR_FALLBACK);
    timed(ctx, "zstd_decode_fallback", ctx->stream, [&] {
        if (!ctx->sw.fz_only) launch_decode(a, p.fallback_grid, r->shape.wide_rows, ctx->stream);
    });
}

// counters, hand-over counts, work cursors and the status column: one stream operation
static int run_clear(znippy_ctx *ctx, znippy_rows *r, const RunPlan &p, const RowsRun &run) {
    hipStream_t s = run.on;
    // (the slot's last user — the run before last — may have had its verify on the auxiliary stream: long done in a steady pipeline)
    if (r->aux_used) HIPCHK(ctx, hipStreamWaitEvent(s, r->ev_done[run.slot], 0));
    if (run.preset) HIPCHK(ctx, hipMemcpyAsync(r->ctl, r->status_init, r->ctl_bytes, hipMemcpyDeviceToDevice, s));
    else HIPCHK(ctx, hipMemsetAsync(r->ctl, 0, r->ctl_bytes, s));
    // (the second hash pass looks at small tiles only when rows were handed over)
    if (p.small_off) HIPCHK(ctx, hipMemsetD32Async((hipDeviceptr_t)r->hand(H_FUSED), (int)r->shape.n, 1, s));
    // ZNIPPY_FZ_ONLY (test hook): a row the parallel paths leave is never decoded and never hashed, and k_verify compares whatever its
    // digest slot holds — in a recycled buffer, or in memory a context of the same process gave back, that can be the row's own right
    // digest of an earlier table, and the row came back verified.  Cleared, the slot never equals a checksum: the row is corrupt, as
    // the hook promises.  (With the serial decoder in place every row with a status >= 0 is hashed: nothing to clear.)
    if (ctx->sw.fz_only && r->shape.n) HIPCHK(ctx, hipMemsetAsync(r->digests, 0, 32 * (size_t)r->shape.n, s));
    return ZNIPPY_OK;
}

// 1) small rows: decode simple frames + hash (+ copy stored rows), one wave per tile; the role-split kernel in front
static int run_small_rows(znippy_ctx *ctx, znippy_rows *r, const RunPlan &p, const RowsRun &run) {
    hipStream_t s = run.on;
    FusedArgs f{};
    f.h = rows_hash_args(ctx, r, p, run);
    f.h.pass = 1;  // PASS_FUSED
    f.blob_size = r->blob_size; f.out_cap = run.out_cap; f.status = r->status;
    f.preset = run.preset;
    f.pending = r->pending; f.pending_count = r->hand(H_FUSED);
    if (run.plain) {  // store-only: one kernel over the plan's small tiles, no diagnostics
        if (p.small) timed(ctx, "decode_small", s, [&] { launch_decode_small(f, s); });
        return ZNIPPY_OK;
    }
    f.dbg = ctx->sw.dbg;
    if (f.dbg & 8) {  // diagnostic: print the previous launch's phase stamps, then reset them
        f.dbg_buf = diag_cycle<8>(ctx, znippy_ctx::DIAG_FUSED, s, nullptr, [](const unsigned long long *h4) {
            if (h4[3]) fprintf(stderr, "[znippy dbg] waves=%llu prologue=%.0f decode=%.0f hash=%.0f | parse+lits=%.0f expand-build=%.0f stream-out=%.0f after-match=%.0f cycles/wave\n", h4[3],
                               (double)h4[0] / h4[3], (double)h4[1] / h4[3], (double)h4[2] / h4[3], (double)h4[6] / h4[3], (double)h4[4] / h4[3], (double)h4[5] / h4[3], (double)h4[7] / h4[3]);
        });
        set_fused_dbg(f.dbg_buf);
    }
    if (f.dbg & 32768) {
        if (!ctx->clk_buf) { (void)hipMalloc(&ctx->clk_buf, roles_clk_bytes(ctx->cus)); (void)hipMemset(ctx->clk_buf, 0, roles_clk_bytes(ctx->cus)); }
        f.dbg_buf = ctx->clk_buf;
    }
    if (f.dbg & (16 | 32 | 64)) set_fused_abl(f.dbg);
    f.lds_pad = ctx->sw.lds_pad;
    const hipStream_t fs = p.lean_mixed ? ctx->aux : s;
    if (p.lean_mixed) {
        HIPCHK(ctx, hipEventRecord(ctx->ev_fork, s));
        HIPCHK(ctx, hipStreamWaitEvent(ctx->aux, ctx->ev_fork, 0));
    }
    if (p.roles) {
        f.cursor = r->cur(CUR_ROLES);
        f.tile_list = r->slow_list;
        f.tile_count = r->hand(H_TILES);
        timed(ctx, run.verify ? "verify_roles" : "decode_verify_roles", fs, [&] { launch_fused_roles(f, ctx->cus, fs, run.verify); });
    }
    if (p.small) timed(ctx, run.verify ? "verify_small" : "decode_verify_fused", fs, [&] { launch_fused_small(f, fs, p.small_grid_cap, run.verify); });
    if (p.lean_mixed) HIPCHK(ctx, hipEventRecord(ctx->ev_join, ctx->aux));  // (joined in front of the verify)
    return ZNIPPY_OK;
}

// Round-2 two-phase path for foreign frames (what the block items gave up on): entropy-decode every block at once, then
// execute frame by frame.  Behind the block items and BESIDE the general decoder on the main stream: both are a few
// long-lived waves per frame, neither fills the chip (real text, libzstd -19 frames: the two used to run back to back,
// 7.0 + 10.6 ms).
static void run_two_phase(znippy_ctx *ctx, znippy_rows *r, const RowsRun &run, hipStream_t ba) {
    FzArgs z{};
    z.cand_row = r->cand_row; z.cand_fzbase = r->fz_base; z.cand_fzcap = r->fz_cap; z.n_cand = r->shape.n_cand;
    z.it_cand = r->fz_it_cand; z.total_items = r->shape.fz_total; z.cand_nb = r->fz_nb; z.items = r->fz_items;
    fill_row_args(z, r, run);
    z.row_flag = r->row_flag;
    z.lit_pool = ctx->fz_lit_pool; z.lit_cap = ctx->fz_lit_cap; z.seq_pool = ctx->fz_seq_pool; z.seq_cap = ctx->fz_seq_cap;
    z.pool_used = r->ctl_at<unsigned long long>(CTL_FZ_POOL);  // [lit bytes, seq records], zeroed with the control block
    z.cursor = r->cur(CUR_FZ);
    if (ctx->sw.ddbg)  // diagnostic: where the previous run's execute kernel spent its cycles
        z.dbg = diag_cycle<32>(ctx, znippy_ctx::DIAG_FZ, ctx->stream, ba, [](const unsigned long long *h) {
            if (h[0]) fprintf(stderr, "[znippy ddbg] fz exec: frames=%llu groups=%llu seqs=%llu big=%llu rounds=%llu flushes=%llu histreads=%llu rep_groups=%llu | kcycles/frame: total=%.0f records=%.0f rep+scan=%.0f big=%.0f flush=%.0f histread=%.0f lits=%.0f matches=%.0f tail=%.0f\n",
                              h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], h[8] / 1e3 / h[0], h[9] / 1e3 / h[0], h[10] / 1e3 / h[0], h[11] / 1e3 / h[0],
                              h[12] / 1e3 / h[0], h[13] / 1e3 / h[0], h[14] / 1e3 / h[0], h[15] / 1e3 / h[0], h[16] / 1e3 / h[0]);
            if (h[20]) fprintf(stderr, "[znippy ddbg] fz entropy: blocks=%llu seqs=%llu | kcycles/block: literal tree=%.0f literal table+streams=%.0f sequence tables=%.0f sequence decode=%.0f\n",
                               h[20], h[25], h[21] / 1e3 / h[20], h[22] / 1e3 / h[20], h[23] / 1e3 / h[20], h[24] / 1e3 / h[20]);
        });
    launch_fz_scan(z, r->fz_work, r->cur(CUR_FZ_WORK), ba);
    timed(ctx, "zstd_foreign_entropy", ba, [&] { launch_fz_entropy(z, ctx->cus, r->fz_work, r->cur(CUR_FZ_WORK), ba); });
    timed(ctx, "zstd_foreign_execute", ba, [&] { launch_fz_exec(z, ba); });
}

// 2a) block items: frames of >= 2 blocks, every block a work item, on the auxiliary stream beside the decoders of 2b (each
//     is latency-bound on its own and leaves most of the chip idle) — or in front of them on the main stream (one_stream)
static int run_block_items(znippy_ctx *ctx, znippy_rows *r, const RunPlan &p, const RowsRun &run) {
    hipStream_t s = ctx->stream;
    const hipStream_t ba = p.one_stream ? s : ctx->aux;
    const BlockScanArgs b = rows_scan_args(r, run);
    if (!p.one_stream) {
        HIPCHK(ctx, hipEventRecord(ctx->ev_fork, s));
        HIPCHK(ctx, hipStreamWaitEvent(ba, ctx->ev_fork, 0));
    }
    timed(ctx, "zstd_block_scan", ba, [&] { launch_scan_blocks(b, ba); });
    if (p.fused_blocks) {  // blocks of the common shape: written and hashed in one go, skipped by the block decoder and the second hash pass
        HIPCHK(ctx, hipMemsetAsync(r->tile_done, 0, r->done_bytes, ba));
        FusedBlocksArgs fb{};
        fb.h = rows_hash_args(ctx, r, p, run);
        fb.h.pass = 0;  // PASS_ALL
        fb.blob_size = r->blob_size;
        fb.bt_tile = r->bt_tile; fb.bt_item = r->bt_item; fb.n_bt = r->shape.n_bt;
        fb.item_src = r->item_src; fb.row_flag = r->row_flag;
        fb.tile_done = r->tile_done; fb.item_done = r->item_done;
        fb.dbg = ctx->sw.dbg;
        if (run.plain) timed(ctx, "decode_blocks", ba, [&] { launch_decode_blocks(fb, ba); });
        else timed(ctx, run.verify ? "verify_blocks" : "decode_verify_fused_blocks", ba, [&] { launch_fused_blocks(fb, ba, run.verify); });
        launch_compact_items(r->item_done, r->shape.n_items, r->todo, r->hand(H_ITEMS), ba);
    }
    DecodeArgs a{};
    fill_row_args(a, r, run);
    a.block_mode = 1;
    a.item_row = r->item_row; a.item_k = r->item_k; a.item_src = r->item_src; a.n_items = r->shape.n_items; a.row_flag = r->row_flag;
    a.item_done = p.fused_blocks ? r->item_done : nullptr;
    a.todo = p.fused_blocks ? r->todo : nullptr; a.n_todo = r->hand(H_ITEMS);
    a.pending_count = r->hand(H_FUSED);
    a.compressed = r->compressed;
    a.n_rows = r->shape.n; a.cursor = r->cur(CUR_ITEMS);
    a.lit_scratch = ctx->lit_scratch_b;
    if (ctx->sw.ddbg)  // diagnostic: phase shares of the previous block-item launch
        a.dbg = diag_cycle<8>(ctx, znippy_ctx::DIAG_ITEMS, s, ba, [](const unsigned long long *h) {
            if (h[0]) fprintf(stderr, "[znippy ddbg] block items=%llu  cycles per item: literals=%.0f seq-tables=%.0f seq-decode=%.0f execute=%.0f tail=%.0f\n", h[0],
                              (double)h[1] / h[0], (double)h[2] / h[0], (double)h[3] / h[0], (double)h[4] / h[0], (double)h[5] / h[0]);
        });
    if (p.block_decoder) timed(ctx, "zstd_decode_blocks", ba, [&] { launch_decode(a, p.items_grid, false, ba); });
    if (p.two_phase) run_two_phase(ctx, r, run, ba);
    if (!p.one_stream) HIPCHK(ctx, hipEventRecord(ctx->ev_join, ctx->aux));
    return ZNIPPY_OK;
}

static BxArgs rows_bx_args(znippy_ctx *ctx, const znippy_rows *r, const RunPlan &p, const RowsRun &run) {
    BxArgs x{};
    x.list_a = r->list_a; x.n_list_a = r->shape.n_list_a;
    x.pending = r->pending; x.pending_count = r->hand(H_FUSED);
    if (p.small_off) {  // every row is the batch path's: its list is all rows, nothing was handed over (a word that stays zero)
        x.list_a = r->all_rows; x.n_list_a = r->shape.n;
        x.pending_count = r->ctl_at<uint32_t>(CTL_RX, RX_ZERO);
    }
    x.bc_row = r->cand_row; x.n_bc = r->shape.n_cand;
    fill_row_args(x, r, run);
    x.row_flag = r->row_flag;
    x.cand_row = r->bx_cand_row; x.cand_base = r->bx_cand_base; x.cand_nb = r->bx_cand_nb; x.slot_cap = r->shape.bx_slots;
    x.items = r->bx_items; x.prep = r->bx_prep; x.item_cap = r->shape.bx_item_cap;
    x.ctr = r->ctl_at<uint32_t>(CTL_BX_CTR);
    x.huf_list = r->bx_huf_list; x.seq_list = r->bx_seq_list; x.sort_tmp = r->bx_sort_tmp;
    x.lit_pool = ctx->fz_lit_pool; x.lit_cap = ctx->fz_lit_cap; x.seq_pool = ctx->fz_seq_pool; x.seq_cap = ctx->fz_seq_cap;
    x.fse_pool = ctx->bx_fse_pool; x.fse_cap = ctx->bx_fse_cap; x.huf_pool = ctx->bx_huf_pool; x.huf_cap = ctx->bx_huf_cap;
    x.pool_used = r->ctl_at<unsigned long long>(CTL_BX_POOL);
    x.pending2 = r->pending2; x.pending2_count = r->hand(H_SERIAL);
    x.big_seq = p.big_seq;
    if (p.rx) {
        x.rx_ptr = ctx->rx_pool; x.rx_cap = ctx->rx_cap; x.rx_chunk = ctx->rx_chunk; x.rx_cdone = ctx->rx_cdone;
        x.rx_base = r->rx_base; x.rx_fail = r->rx_fail; x.rx_blk = r->rx_blk; x.rx_list = r->rx_list;
        x.rx_pending = r->ctl_at<uint32_t>(CTL_RX);
        x.rx_bound = p.rx_bound;
        x.rx_min = r->shape.rx_min;
    }
    x.xxh_on = p.xxh;
    x.xxh_forms = r->shape.xxh_forms; x.cand_ck = r->bx_cand_ck; x.xxh_stat = r->ctl_at<unsigned long long>(CTL_BX_XXH);
    x.small_frames = p.small_frames;
    if (ctx->sw.ddbg)  // diagnostic: where the previous run's table kernel spent its waves' time
        x.dbg = diag_cycle<128>(ctx, znippy_ctx::DIAG_BX, ctx->stream, nullptr, [](const unsigned long long *h) {
            if (h[64]) {
                const unsigned long long *e = h + 64;
                fprintf(stderr, "[znippy ddbg] batch execute: frames=%llu groups=%llu seqs=%llu big=%llu rounds=%llu flushes=%llu histreads=%llu | kcycles/frame: total=%.1f records=%.1f rep+scan=%.1f big=%.1f flush=%.1f histread=%.1f lits=%.1f matches=%.1f tail=%.1f\n",
                        e[0], e[1], e[2], e[3], e[4], e[5], e[6], e[8] / 1e3 / e[0], e[9] / 1e3 / e[0], e[10] / 1e3 / e[0], e[11] / 1e3 / e[0], e[12] / 1e3 / e[0], e[13] / 1e3 / e[0],
                        e[14] / 1e3 / e[0], e[15] / 1e3 / e[0], e[16] / 1e3 / e[0]);
            }
            if (h[32]) fprintf(stderr, "[znippy ddbg] batch tables: wave passes=%llu  kcycles per pass: literals header + weights=%.1f sequences header=%.1f huffman table=%.1f sequence tables=%.1f\n", h[32],
                               h[33] / 1e3 / h[32], h[34] / 1e3 / h[32], h[35] / 1e3 / h[32], h[36] / 1e3 / h[32]);
        });
    return x;
}
static void bx_stage(znippy_ctx *ctx, const BxArgs &x, BxStage st, hipStream_t on) {
    static const char *const names[10] = {"zstd_batch_scan", "zstd_batch_tables", "zstd_batch_huffman", "zstd_batch_sequences", "zstd_batch_execute", "zstd_batch_finish",
                                          "zstd_batch_sequences_long", "zstd_batch_sort", "zstd_resolve_plan", "zstd_resolve_expand"};
    timed(ctx, names[st], on, [&] { launch_bx_stage(x, ctx->cus, st, on); });
}
// big frames of the batch path: resolved in parallel (every byte a word, pointer jumping) instead of executed by a wave each;
// the frames the plan did not take are executed by a wave each, beside the resolve stages (they share nothing)
static int run_resolve(znippy_ctx *ctx, znippy_rows *r, const BxArgs &x) {
    hipStream_t s = ctx->stream;
    bx_stage(ctx, x, BX_RX_PLAN, s);
    if (ctx->sw.trace) {
        uint32_t g[16];
        unsigned long long pu[16];
        (void)hipMemcpy(g, r->ctl + CTL_BX_CTR.at, CTL_BX_CTR.bytes, hipMemcpyDeviceToHost);
        (void)hipMemcpy(pu, r->ctl + CTL_BX_POOL.at, CTL_BX_POOL.bytes, hipMemcpyDeviceToHost);
        fprintf(stderr, "[znippy trace] resolve plan: slots %u items %u list %u frames %u words %llu extent %llu cap %llu item_cap %u\n", g[0], g[1], g[9], g[11], pu[10], pu[11],
                (unsigned long long)ctx->rx_cap, r->shape.bx_item_cap);
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev_fork, s));
    HIPCHK(ctx, hipStreamWaitEvent(ctx->aux, ctx->ev_fork, 0));
    bx_stage(ctx, x, BX_EXEC, ctx->aux);
    HIPCHK(ctx, hipEventRecord(ctx->ev_join, ctx->aux));
    bx_stage(ctx, x, BX_RX_EXPAND, s);
    static const char *const jump_names[12] = {"zstd_resolve_jump_0", "zstd_resolve_jump_1", "zstd_resolve_jump_2", "zstd_resolve_jump_3", "zstd_resolve_jump_4", "zstd_resolve_jump_5",
                                               "zstd_resolve_jump_6", "zstd_resolve_jump_7", "zstd_resolve_jump_8", "zstd_resolve_jump_9", "zstd_resolve_jump_10", "zstd_resolve_jump_11"};
    static_assert(zn::RX_ROUNDS <= 12, "names");
    if (!ctx->sw.ddbg) ktime_begin(ctx, "zstd_resolve_jump", s);
    for (int rd = 0; rd < (int)zn::RX_ROUNDS; rd++) {
        if (ctx->sw.ddbg) ktime_begin(ctx, jump_names[rd], s);  // diagnostic: every round by itself
        launch_bx_stage(x, ctx->cus, BX_RX_JUMP + rd, s);
        if (ctx->sw.ddbg) ktime_end(ctx, s);
    }
    if (!ctx->sw.ddbg) ktime_end(ctx, s);
    timed(ctx, "zstd_resolve_store", s, [&] { launch_bx_stage(x, ctx->cus, BX_RX_STORE, s); });
    HIPCHK(ctx, hipStreamWaitEvent(s, ctx->ev_join, 0));
    return ZNIPPY_OK;
}
// 2b) batch path: every frame that is still undecoded — big single-block rows, what the fused kernel handed over, block
//     candidates the block-item path flagged — goes through the lane-per-block kernels in ONE pass (the more blocks, the
//     fuller their waves), behind the block items; the serial decoder takes what they leave.
static int run_batch_path(znippy_ctx *ctx, znippy_rows *r, const RunPlan &p, const RowsRun &run) {
    hipStream_t s = ctx->stream;
    const DecodeArgs a = rows_decode_args(ctx, r, run);
    if (p.items) {
        HIPCHK(ctx, hipStreamWaitEvent(s, ctx->ev_join, 0));
        launch_finish_blocks(rows_scan_args(r, run), s, true);  // unflagged candidates are done; flagged ones wait for the batch path's verdict
    }
    const BxArgs x = rows_bx_args(ctx, r, p, run);
    bx_stage(ctx, x, BX_SCAN, s);
    bx_stage(ctx, x, BX_PREP, s);
    bx_stage(ctx, x, BX_SORT, s);
    // the long chains (blocks of >= BX_BIG_SEQ sequences, a wave each) run on the auxiliary stream beside the Huffman
    // streams and the lane-per-block sequence kernel: each is a few hundred long-lived waves at most
    HIPCHK(ctx, hipEventRecord(ctx->ev_fork, s));
    HIPCHK(ctx, hipStreamWaitEvent(ctx->aux, ctx->ev_fork, 0));
    bx_stage(ctx, x, BX_FSE_WAVE, ctx->aux);
    HIPCHK(ctx, hipEventRecord(ctx->ev_join, ctx->aux));
    // ... and the lane-per-block sequence kernel beside the Huffman streams on a third stream (the write side's copy
    // stream, idle here): the two touch different pools and different fields of a block's record.  A small table is
    // its longest chains: the image's source text had Huffman 2.5 + sequences 1.8 ms in a row beside 3.5 ms of long chains.
    if (p.third) {
        HIPCHK(ctx, hipStreamWaitEvent(ctx->copy, ctx->ev_fork, 0));
        bx_stage(ctx, x, BX_FSE, ctx->copy);
        HIPCHK(ctx, hipEventRecord(ctx->ev_join2, ctx->copy));
    }
    bx_stage(ctx, x, BX_HUF, s);
    if (!p.third) bx_stage(ctx, x, BX_FSE, s);
    HIPCHK(ctx, hipStreamWaitEvent(s, ctx->ev_join, 0));
    if (p.third) HIPCHK(ctx, hipStreamWaitEvent(s, ctx->ev_join2, 0));
    if (p.rx) { const int rc = run_resolve(ctx, r, x); if (rc) return rc; }
    else bx_stage(ctx, x, BX_EXEC, s);
    // frames with a content checksum that were decoded above: a wrong trailer makes the frame undecoded again (the finish stage lists it)
    if (x.xxh_on) timed(ctx, "zstd_batch_checksum", s, [&] { launch_bx_stage(x, ctx->cus, BX_XXH, s); });
    bx_stage(ctx, x, BX_FINISH, s);
    decode_rest(ctx, r, p, a);
    return ZNIPPY_OK;
}
// 2b') round-2 flow (no batch path: ZNIPPY_NO_BX, no pools, or a table whose last run handed nothing over): the serial
//      decoder takes the host's list and what the fused kernel hands over, beside the block items on the auxiliary stream —
//      or behind them when nothing is expected; frames the block path gives up on are decoded by a second launch afterwards.
static int run_serial_flow(znippy_ctx *ctx, znippy_rows *r, const RunPlan &p, const RowsRun &run) {
    hipStream_t s = ctx->stream;
    const DecodeArgs a = rows_decode_args(ctx, r, run);
    if (p.behind) {
        if (!p.one_stream) HIPCHK(ctx, hipStreamWaitEvent(s, ctx->ev_join, 0));
        launch_finish_blocks(rows_scan_args(r, run), s, false);
    }
    if (p.lean_blocks) return ZNIPPY_OK;
    timed(ctx, "zstd_decode_general", s, [&] { launch_decode(a, p.general_grid, r->shape.wide_rows, s); });
    if (!p.items) return ZNIPPY_OK;
    if (!p.behind) {  // join (block items and the foreign-frame path on the auxiliary stream), then what both gave up on
        HIPCHK(ctx, hipStreamWaitEvent(s, ctx->ev_join, 0));
        launch_finish_blocks(rows_scan_args(r, run), s, false);
    }
    decode_rest(ctx, r, p, a);
    return ZNIPPY_OK;
}

// 3) second hash pass: slices of big rows + rows the decoders finished (stored_only: every tile), then the big rows' trees
static void run_second_hash(znippy_ctx *ctx, znippy_rows *r, const RunPlan &p, const RowsRun &run) {
    hipStream_t s = ctx->stream;
    HashArgs h = rows_hash_args(ctx, r, p, run);
    h.pass = p.stored_only ? 0 : 2;  // PASS_ALL : PASS_SECOND
    h.tile_done = p.hash_skips_done ? r->tile_done : nullptr;
    timed(ctx, run.verify ? "blake3_hash_only" : "blake3_second_pass", s, [&] { launch_hash_tiles(h, s); });
    if (p.merge_big)
        timed(ctx, "blake3_merge_big", s, [&] {
            launch_merge_big(r->plan.big, r->plan.n_big, r->plan.tile_cv, r->digests, r->plan.grp_big, r->plan.grp_k, r->plan.n_grp, r->plan.max_cvs, s);
        });
}

// 3') decode-only runs: no hash pass — what is left of it is the copy of the stored rows no kernel in front has written (stored rows
//     above a tile; stored_only: every row)
static void run_copy_stored(znippy_ctx *ctx, znippy_rows *r, const RunPlan &p, const RowsRun &run) {
    if (!p.copy_stored) return;
    const HashArgs h = rows_hash_args(ctx, r, p, run);
    timed(ctx, "copy_stored", ctx->stream, [&] { launch_copy_stored(h, p.stored_only, ctx->stream); });
}

// 4) verify (a run that left stages out: its lists must be empty, or the counters come back flagged), mirror copy, event
static int run_verify(znippy_ctx *ctx, znippy_rows *r, const RunPlan &p, const RowsRun &run) {
    hipStream_t s = run.on;
    if (p.lean_mixed) HIPCHK(ctx, hipStreamWaitEvent(s, ctx->ev_join, 0));
    // (a lean run's) verify, result copy and the run's event go to the auxiliary stream behind an event, and the next run's kernel
    // follows this run's directly.  The slot's next run is ordered behind ev_done (run_clear).
    if (p.verify_aux) {
        HIPCHK(ctx, hipEventRecord(r->ev_main[run.slot], s));
        if (run.lane_ev) HIPCHK(ctx, hipEventRecord(run.lane_ev, s));  // (what later lane runs and the main stream wait for: lane_begin)
        s = ctx->aux;
        HIPCHK(ctx, hipStreamWaitEvent(s, r->ev_main[run.slot], 0));
        r->aux_used = true;
    }
    // (decode-only: the counters pass alone — no checksum column, no digest read, every decoded row counts as verified)
    timed(ctx, run.plain ? "count_rows" : "verify", s, [&] {
        launch_verify(r->digests, run.plain ? nullptr : r->checksum, r->usize, r->status, r->shape.n, r->row_begin, r->counters, r->corrupt, r->corrupt_cap, s,
                      p.check_lists ? r->ctl_at<uint32_t>(CTL_HAND) : nullptr, p.lists_small ? LEAN_SMALL : LEAN_BLOCKS);
    });
    HIPCHK(ctx, hipMemcpyAsync(r->h_counters + 16 * run.slot, r->counters, CTL_MIRROR, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipEventRecord(r->ev_done[run.slot], s));
    HIPCHK(ctx, hipGetLastError());
    return ZNIPPY_OK;
}

// A lean run on a context with run lanes: picks the run's stream (run k of a table: lane k & 1; lane 0 is the main stream) and
// queues on it whatever the run has to wait for — never more than an event wait, and nothing at all in a steady pipeline.
//  - Main-stream work queued since the last lane run (main_dirty): a mark is recorded on the main stream in front of this run and
//    a run on lane 1 waits for it; a run on lane 0 stands behind it anyway and leaves the wait to the next run on lane 1.
//  - The latest run on the OTHER stream that is older than the predecessor: waited for unless it has ended (one event query).
//    Runs older than that on the other stream ended before it, older runs on this stream end before this run starts, so only
//    the predecessor can still be executing when this run starts (the same slot's last run is behind ev_done besides).
//  - The predecessor: on this stream the run stands behind it whatever the rule says.  On the other stream
//    zn_runs_may_overlap decides (host/run_overlap.cc): beside it, or behind its event.
// The main stream does NOT wait for a run on lane 1 here — the next run on lane 0 would stand behind it; lanes_close does, in front
// of anything else the context queues.
// What two lean runs side by side share, checked against the kernels:
//  - slow_list is one per table and both runs' role-split kernels may append to it, each with its own count (H_TILES of its slot,
//    at most the tile count, so no append leaves the list).  No lean run reads the list: a run that appended comes back flagged,
//    and rows_settle synchronises every stream and runs it again in full, by itself.
//  - No pool of the context: the role-split kernel reads blobs and writes rows (k_fused_roles<true>) or hashes the periodic shape
//    in LDS and writes digests only (<false>, a verify-only run: its d_out, the verify scratch, is never dereferenced — rows of
//    any other shape go to slow_list, i.e. to a full run).
static int lane_begin(znippy_ctx *ctx, znippy_rows *r, unsigned slot, hipStream_t *on, hipEvent_t *record) {
    const auto &ra = r->run_args[slot];
    const bool on_lane = (slot & 1) != 0;
    const unsigned si = on_lane ? 1 : 0, oi = si ^ 1;
    const hipStream_t s = on_lane ? ctx->lane : ctx->stream;
    const zn_run_desc d{r, slot, 1, (uint8_t)ra.verify, (uint64_t)(uintptr_t)ra.blobs, ra.base, ra.blob_cap, (uint64_t)(uintptr_t)ra.out, ra.cap};
    auto wait_on = [&](hipEvent_t e) {
        if (!on_lane && e == ctx->lane_join) ctx->lane_join = nullptr;  // (the main stream is behind that run now)
        return hipStreamWaitEvent(s, e, 0);
    };
    if (ctx->main_dirty) {  // (lanes_close has left no predecessor and no history)
        HIPCHK(ctx, hipEventRecord(ctx->ev_mark, ctx->stream));
        ctx->main_dirty = false; ctx->mark_pending = true;
        ctx->lane_stats[2]++;
    }
    if (on_lane && ctx->mark_pending) {
        HIPCHK(ctx, hipStreamWaitEvent(s, ctx->ev_mark, 0));
        ctx->mark_pending = false;
    }
    const znippy_ctx::LaneRun p0 = ctx->lane_prev;
    const bool p0_other = p0.valid && p0.on_lane != on_lane;
    // the latest run on the other stream that is older than the predecessor
    const znippy_ctx::LaneRun &older = ctx->lane_hist[oi][p0_other ? 1 : 0];
    if (older.valid) {
        if (hipEventQuery(older.ev) == hipSuccess) (void)0;  // it has ended, and with it everything in front of it on that stream
        else {
            (void)hipGetLastError();  // (hipErrorNotReady)
            HIPCHK(ctx, wait_on(older.ev));
            ctx->lane_stats[4]++;
        }
    }
    const bool beside = p0_other && zn_runs_may_overlap(&p0.d, &d);
    if (p0_other && !beside) HIPCHK(ctx, wait_on(p0.ev));
    ctx->lane_stats[beside ? 0 : 1]++;  // beside: on another stream than the predecessor and with no wait for it
    // The run's event enters predecessor, history and lane_join HERE, before run_verify records it: nothing between the two
    // queues a lane run, and a run that fails in between ends in rows_abandon, which closes the lanes (no entry survives) and
    // synchronises.  (The event taken is the one just shifted out of this stream's history.)
    hipEvent_t ev = ctx->lane_ev[si][ctx->lane_n[si]++ & 1];
    ctx->lane_prev = znippy_ctx::LaneRun{d, ev, on_lane, true};
    ctx->lane_hist[si][1] = ctx->lane_hist[si][0];
    ctx->lane_hist[si][0] = ctx->lane_prev;
    if (on_lane) { ctx->lane_join = ev; r->lane_used = true; }
    *on = s;
    *record = ev;
    return ZNIPPY_OK;
}

// Queues one run of the table with the given arguments; its counters land in mirror slot `slot` and ev_done[slot] marks its
// end.  run_seq is the caller's (znippy_decode_verify_rows_async advances it, a repeat inside rows_settle does not).  Every
// allocation the run needs is made before its first stream operation on the table (*queued): an error return after that
// point is a HIP runtime error, which the caller turns into a table without a readable run (rows_abandon).
// verify: a verify-only run (d_out / out_cap are not looked at: the run's output region is the context's scratch as it is NOW — a repeat
// inside rows_settle finds the region wherever a later run of another table has moved it).
static int rows_launch(znippy_ctx *ctx, znippy_rows *r, const void *d_blobs, uint64_t blob_base, void *d_out, uint64_t out_cap,
                       unsigned slot, bool verify, bool plain, bool *queued = nullptr) {
    ctx->n_ktimes = 0;
    int rc = ensure_decoder(ctx);
    if (!rc && verify) {
        rc = rows_verify_slots(ctx, r);
        if (!rc) rc = ensure_verify_scratch(ctx, r->vs_bytes);
        d_out = ctx->vs_pool; out_cap = r->vs_bytes;
    }
    if (!rc) rc = rows_validate(ctx, r, blob_base, out_cap, verify);
    if (!rc && r->shape.fz_total) rc = ensure_fz_pools(ctx, r->shape.fz_bytes, r->shape.fz_total);
    if (!rc && r->shape.bx_slots) {
        rc = ensure_fz_pools(ctx, r->shape.bx_bytes, r->shape.bx_item_cap);
        if (!rc) rc = ensure_bx_pools(ctx, r->shape.bx_bytes, r->shape.bx_item_cap);
        if (!rc && r->rx_base && rows_route_hint(r->hints, plain) != 0) rc = ensure_rx_pool(ctx, r->shape.rx_words);
        if (!rc && ctx->batch_checksums && !r->bx_cand_ck && tmalloc(ctx, &r->bx_cand_ck, 4 * (size_t)r->shape.bx_slots) != hipSuccess) rc = ZNIPPY_E_NOMEM;
    }
    if (rc) return rc;
    if (r->shape.n_cand && ensure_decoder_b(ctx)) return ZNIPPY_E_NOMEM;
    if (r->run_seq && rows_route_hint(r->hints, plain) < 0 && r->shape.n) {  // a run of this table has finished meanwhile?
        const unsigned last = (unsigned)((r->run_seq - 1) & 1);
        const bool last_plain = r->run_args[last].plain;  // (a decode-only run teaches the table's own hints nothing)
        if (last_plain && !plain) (void)0;
        else if (hipEventQuery(r->ev_done[last]) != hipSuccess) (void)hipGetLastError();
        else if (last_plain) rows_note_plain(r->shape, r->hints, r->mirror_hand(last));
        else rows_note_hint(r->shape, r->hints, r->mirror_hand(last));
    }
    RowsRun run{d_blobs, blob_base, d_out, out_cap, r->hints.n_bad ? 1 : 0, slot, verify, plain, ctx->stream, nullptr};
    const RunPlan p = rows_plan(r->shape, r->hints, rows_run_env(ctx, r, d_out), run.preset, verify, plain);
    if (p.small_off && !r->all_rows) {
        if (tmalloc(ctx, &r->all_rows, 4 * (size_t)r->shape.n) != hipSuccess) return ZNIPPY_E_NOMEM;
        hipLaunchKernelGGL(k_iota32, dim3((r->shape.n + 255) / 256), dim3(256), 0, ctx->stream, r->all_rows, r->shape.n);
    }
    { auto &ra = r->run_args[slot]; ra.blobs = d_blobs; ra.base = blob_base; ra.out = verify ? nullptr : d_out; ra.cap = verify ? 0 : out_cap; ra.blob_cap = r->blob_cap; ra.verify = verify; ra.plain = plain; }
    r->select(slot);
    if (queued) *queued = true;
    if (p.lean && ctx->lanes_on) {
        if ((rc = lane_begin(ctx, r, slot, &run.on, &run.lane_ev))) return rc;
    } else {
        if (p.lean) ctx->lane_stats[3]++;  // a lean run kept off the lanes: a caller's stream, or a switch
        lanes_close(ctx);                  // what this run queues on the main stream stands behind every lane run
    }
    if ((rc = run_clear(ctx, r, p, run)) || p.empty) return rc;
    if (!p.small_off && !p.stored_only && (rc = run_small_rows(ctx, r, p, run))) return rc;
    if (p.items && (rc = run_block_items(ctx, r, p, run))) return rc;
    if (p.decoders && (rc = p.bx ? run_batch_path(ctx, r, p, run) : run_serial_flow(ctx, r, p, run))) return rc;
    if (plain) run_copy_stored(ctx, r, p, run);
    else if (!p.lean) run_second_hash(ctx, r, p, run);
    return run_verify(ctx, r, p, run);
}

// A run that failed after its first stream operation: whatever it queued on the auxiliary stream is joined back into the
// main one and waited for, and the table forgets its runs (the control block, the status column and one mirror slot may hold
// a part of the failed run): results calls see no run until the next one is queued, and that one runs in full.
static void rows_abandon(znippy_ctx *ctx, znippy_rows *r);
static int rows_queue(znippy_ctx *ctx, znippy_rows *r, const void *d_blobs, uint64_t blob_base, void *d_out, uint64_t out_cap, bool verify, bool plain = false) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    { const int prc = poison_enter(ctx); if (prc) return prc; }
    bool queued = false;
    const int rc = rows_launch(ctx, r, d_blobs, blob_base, d_out, out_cap, (unsigned)(r->run_seq & 1), verify, plain, &queued);
    if (rc && queued) rows_abandon(ctx, r);
    if (rc) return rc;
    r->run_seq++;
    return ZNIPPY_OK;
}
static void rows_abandon(znippy_ctx *ctx, znippy_rows *r) {
    lanes_close(ctx);
    (void)lanes_sync(ctx);
    if (hipEventRecord(ctx->ev_join, ctx->aux) == hipSuccess) (void)hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0);
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipGetLastError();
    r->run_seq = 0;
    rows_force_full(r->hints);
}

int znippy_decode_verify_rows_async(znippy_ctx *ctx, znippy_rows *r, const void *d_blobs,
                                    uint64_t blob_base, void *d_out, uint64_t out_cap) {
    if (!ctx_enter(ctx, ENTER_RUN)) return ZNIPPY_E_INVAL;
    if (!ctx || !r || r->ctx != ctx) return ZNIPPY_E_INVAL;
    if (r->no_out) return ZNIPPY_E_INVAL;  // created without output offsets: verify-only
    if (r->shape.n && (!d_blobs || !d_out)) return ZNIPPY_E_INVAL;
    return rows_queue(ctx, r, d_blobs, blob_base, d_out, out_cap, false);
}

// The same run without a hash (znippy_hip.h): every row is written where a decode run writes it and no digest is computed or compared.
int znippy_decode_rows_async(znippy_ctx *ctx, znippy_rows *r, const void *d_blobs, uint64_t blob_base, void *d_out, uint64_t out_cap) {
    if (!ctx_enter(ctx, ENTER_RUN)) return ZNIPPY_E_INVAL;
    if (!ctx || !r || r->ctx != ctx) return ZNIPPY_E_INVAL;
    if (r->no_out) return ZNIPPY_E_INVAL;  // created without output offsets: verify-only
    if (r->shape.n && (!d_blobs || !d_out)) return ZNIPPY_E_INVAL;
    return rows_queue(ctx, r, d_blobs, blob_base, d_out, out_cap, false, true);
}

// The same run without an output: every row is decoded as far as hashing it needs, hashed and compared, and nothing is written
// that no kernel reads back (znippy_hip.h).  A run like any other in the table's sequence.
int znippy_verify_rows_async(znippy_ctx *ctx, znippy_rows *r, const void *d_blobs, uint64_t blob_base) {
    if (!ctx_enter(ctx, ENTER_RUN)) return ZNIPPY_E_INVAL;
    if (!ctx || !r || r->ctx != ctx) return ZNIPPY_E_INVAL;
    if (r->shape.n && !d_blobs) return ZNIPPY_E_INVAL;
    return rows_queue(ctx, r, d_blobs, blob_base, nullptr, 0, true);
}

int znippy_rows_verify_scratch(znippy_ctx *ctx, znippy_rows *r, const void **d_base, uint64_t *bytes, uint64_t *row_offset) {
    if (!ctx_enter(ctx)) return ZNIPPY_E_INVAL;
    if (!ctx || !r || r->ctx != ctx || !d_base || !bytes) return ZNIPPY_E_INVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = rows_verify_slots(ctx, r);
    if (!rc) rc = ensure_verify_scratch(ctx, r->vs_bytes);
    if (rc) return rc;
    *d_base = r->vs_bytes ? ctx->vs_pool : nullptr;
    *bytes = r->vs_bytes;
    if (row_offset && r->shape.n) {
        std::vector<uint8_t> comp(r->shape.n);
        std::vector<uint64_t> len(r->shape.n);
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        HIPCHK(ctx, hipMemcpy(row_offset, r->vs_off, 8 * (size_t)r->shape.n, hipMemcpyDeviceToHost));
        HIPCHK(ctx, hipMemcpy(comp.data(), r->compressed, r->shape.n, hipMemcpyDeviceToHost));
        HIPCHK(ctx, hipMemcpy(len.data(), r->usize, 8 * (size_t)r->shape.n, hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < r->shape.n; i++)
            if (!comp[i] || !len[i]) row_offset[i] = ~0ull;
    }
    return ZNIPPY_OK;
}

// A lean run whose lists were not empty after all (counters[7] set by k_verify) is run again in full with the arguments IT was
// given (run_args[slot]: a caller that alternates buffers gets the right buffer completed), its counters into its own mirror
// slot; run_seq does not move, so the caller's lagged reads keep counting the runs it queued.  When a later run stands behind
// it (run k read with lag 1 while run k + 1 was queued), that later run — the latest — is run again in full as well, after the
// first: whatever it was (lean and flagged too, lean and clean, or sharing d_out with run k), its bytes and counters are
// complete before any results call hands them out, and the table's own outputs (status column, corrupt list, digests) once
// more describe the latest run, as znippy_rows_results and znippy_rows_digests report them.  A full run leaves counters[7]
// clear: no slot is repeated twice.  Only runs over changed blobs get here, so the cost of the second repeat does not matter.
// Called by everything that hands a run's results to the caller.
static int rows_settle(znippy_ctx *ctx, znippy_rows *r, unsigned slot) {
    if (!r->shape.n || !r->run_seq || !(r->h_counters[16 * slot + 7])) return ZNIPPY_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, lanes_sync(ctx));                 // the latest run's kernel may be queued there
    HIPCHK(ctx, hipStreamSynchronize(ctx->aux));  // the latest run's verify may be queued there
    rows_force_full(r->hints);
    { const int prc = poison_enter(ctx); if (prc) return prc; }
    const unsigned latest = (unsigned)((r->run_seq - 1) & 1);
    const unsigned order[2] = {slot, latest};
    for (int i = 0; i < (slot == latest ? 1 : 2); i++) {
        const znippy_rows::RunArgs ra = r->run_args[order[i]];
        r->blob_cap = ra.blob_cap;
        bool queued = false;
        const int rc = rows_launch(ctx, r, ra.blobs, ra.base, ra.out, ra.cap, order[i], ra.verify, ra.plain, &queued);
        if (rc) {
            if (queued) rows_abandon(ctx, r);
            return rc;
        }
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return ZNIPPY_OK;
}

// Counters of the run `lag` runs before the latest one (lag 0 or 1): waits for THAT run only, so a caller that
// keeps two runs in flight reads run k's counters while run k + 1 executes (the read loop reports after the loop,
// not per row: decompress.rs:L195-221).
int znippy_rows_results_lagged(znippy_ctx *ctx, znippy_rows *r, unsigned lag, znippy_verify_counters *counters) {
    if (!ctx_enter(ctx, ENTER_RUN)) return ZNIPPY_E_INVAL;
    if (!ctx || !r || r->ctx != ctx || !counters || lag > 1 || r->run_seq <= lag) return ZNIPPY_E_INVAL;
    uint64_t c[8] = {0};
    if (r->shape.n) {
        const unsigned slot = (unsigned)((r->run_seq - 1 - lag) & 1);
        HIPCHK(ctx, hipEventSynchronize(r->ev_done[slot]));
        { const int rc = rows_settle(ctx, r, slot); if (rc) return rc; }
        memcpy(c, r->h_counters + 16 * slot, 64);
        if (r->run_args[slot].plain) rows_note_plain(r->shape, r->hints, r->mirror_hand(slot));
        else rows_note_hint(r->shape, r->hints, r->mirror_hand(slot));
    }
    counters->total_chunks = c[0]; counters->total_written_bytes = c[1]; counters->verified_bytes = c[2];
    counters->corrupt_bytes = c[3]; counters->corrupt_rows = c[4]; counters->decode_errors = c[5];
    return ZNIPPY_OK;
}

int znippy_rows_results(znippy_ctx *ctx, znippy_rows *r, znippy_verify_counters *counters,
                        uint64_t *corrupt_rows, uint64_t corrupt_cap, int32_t *row_status) {
    if (!ctx_enter(ctx, ENTER_RUN)) return ZNIPPY_E_INVAL;
    if (!ctx || !r) return ZNIPPY_E_INVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (r->lane_used) HIPCHK(ctx, lanes_sync(ctx));
    if (r->aux_used) HIPCHK(ctx, hipStreamSynchronize(ctx->aux));  // the latest run's verify may be queued there
    uint64_t c[8] = {0};
    if (r->shape.n && r->run_seq) {
        { const int rc = rows_settle(ctx, r, (unsigned)((r->run_seq - 1) & 1)); if (rc) return rc; }
        memcpy(c, r->h_counters + 16 * ((r->run_seq - 1) & 1), 64);  // copied by the run itself (pinned)
        const unsigned slot = (unsigned)((r->run_seq - 1) & 1);
        if (r->run_args[slot].plain) rows_note_plain(r->shape, r->hints, r->mirror_hand(slot));
        else rows_note_hint(r->shape, r->hints, r->mirror_hand(slot));
    }
    if (counters) {
        counters->total_chunks = c[0]; counters->total_written_bytes = c[1]; counters->verified_bytes = c[2];
        counters->corrupt_bytes = c[3]; counters->corrupt_rows = c[4]; counters->decode_errors = c[5];
    }
    if (corrupt_rows && corrupt_cap && c[4]) {
        uint64_t k = std::min<uint64_t>(c[4], r->corrupt_cap);
        std::vector<uint64_t> tmp(k);
        HIPCHK(ctx, hipMemcpy(tmp.data(), r->corrupt, 8 * k, hipMemcpyDeviceToHost));
        std::sort(tmp.begin(), tmp.end());
        memcpy(corrupt_rows, tmp.data(), 8 * std::min<uint64_t>(k, corrupt_cap));
    }
    if (row_status && r->shape.n) {
        HIPCHK(ctx, hipMemcpy(row_status, r->status, 4 * (size_t)r->shape.n, hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < r->shape.n; i++)
            if (row_status[i] > 0) row_status[i] = 0;  // internal routing states (1, 2) are successes
    }
    return ZNIPPY_OK;
}

int znippy_decode_verify_rows(znippy_ctx *ctx, znippy_rows *rows, const void *d_blobs,
                              uint64_t blob_base, void *d_out, uint64_t out_cap,
                              znippy_verify_counters *counters, uint64_t *corrupt_rows,
                              uint64_t corrupt_cap, int32_t *row_status) {
    if (!ctx_enter(ctx, ENTER_RUN)) return ZNIPPY_E_INVAL;
    int rc = znippy_decode_verify_rows_async(ctx, rows, d_blobs, blob_base, d_out, out_cap);
    if (rc) return rc;
    return znippy_rows_results(ctx, rows, counters, corrupt_rows, corrupt_cap, row_status);
}

int znippy_decode_rows(znippy_ctx *ctx, znippy_rows *rows, const void *d_blobs, uint64_t blob_base, void *d_out, uint64_t out_cap,
                       znippy_verify_counters *counters, int32_t *row_status) {
    if (!ctx_enter(ctx, ENTER_RUN)) return ZNIPPY_E_INVAL;
    int rc = znippy_decode_rows_async(ctx, rows, d_blobs, blob_base, d_out, out_cap);
    if (rc) return rc;
    return znippy_rows_results(ctx, rows, counters, nullptr, 0, row_status);
}

int znippy_verify_rows(znippy_ctx *ctx, znippy_rows *rows, const void *d_blobs, uint64_t blob_base,
                       znippy_verify_counters *counters, uint64_t *corrupt_rows, uint64_t corrupt_cap, int32_t *row_status) {
    if (!ctx_enter(ctx, ENTER_RUN)) return ZNIPPY_E_INVAL;
    int rc = znippy_verify_rows_async(ctx, rows, d_blobs, blob_base);
    if (rc) return rc;
    return znippy_rows_results(ctx, rows, counters, corrupt_rows, corrupt_cap, row_status);
}

// ---- range reads (znippy_rows_read_ranges) --------------------------------------------------------
// The columns a call validates and plans against, on the host: fetched once per table from the device copies, which hold the
// effective lengths (a stored row's length is its blob).  The same three vectors rows_validate fills for its per-row pass.
static int rows_host_columns(znippy_ctx *ctx, znippy_rows *r) {
    if (!r->shape.n || (!r->h_blob_off.empty() && !r->h_comp.empty())) return ZNIPPY_OK;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    // (into temporaries: a copy that fails leaves the table without a half-filled cache)
    std::vector<uint64_t> bo(r->shape.n), bs(r->shape.n), len(r->shape.n);
    std::vector<uint8_t> comp(r->shape.n);
    HIPCHK(ctx, hipMemcpy(bo.data(), r->blob_off, 8 * (size_t)r->shape.n, hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(bs.data(), r->blob_size, 8 * (size_t)r->shape.n, hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(len.data(), r->usize, 8 * (size_t)r->shape.n, hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(comp.data(), r->compressed, r->shape.n, hipMemcpyDeviceToHost));
    if (r->h_blob_off.empty()) { r->h_blob_off.swap(bo); r->h_blob_size.swap(bs); r->h_len.swap(len); }
    r->h_comp.swap(comp);
    return ZNIPPY_OK;
}

// What a call plans against (host/range_plan.h): the host columns above and, where they exist, the tree's layout and verdicts.
static RrTable rows_table_view(const znippy_rows *r) {
    return RrTable{r->shape.n, r->row_begin, r->blob_cap, r->h_blob_off.data(), r->h_blob_size.data(), r->h_len.data(), r->h_comp.data(),
                   r->tree_first.data(), r->tree_first.size(), r->tree_accept.data(), r->tree_accept.size()};
}

// The checksum column on the host (verified range reads give the private tables of their whole-row passes the rows' checksums).
static int rows_host_checksum(znippy_ctx *ctx, znippy_rows *r) {
    if (!r->shape.n || !r->checksum || !r->h_checksum.empty()) return ZNIPPY_OK;
    std::vector<uint8_t> ck((size_t)32 * r->shape.n);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipMemcpy(ck.data(), r->checksum, ck.size(), hipMemcpyDeviceToHost));
    r->h_checksum.swap(ck);
    return ZNIPPY_OK;
}

// Whole rows into the range scratch: a private table over the compact columns of `sel`, one decode-only run of it, the rows' verdicts.
// The run's kernels are bracketed as one entry of the kernel times (range_decode_rows).
// `verify` (verified range reads): the private table gets the rows' checksums and the run is a decode + verify run; a row whose digest
// is not its checksum gets ZNIPPY_E_DIGEST.  `stored`: the rows are stored rows and the run is a verify-only run, which hashes them
// where they lie in the blob region (nothing lands in the scratch).
static int rr_decode_whole(znippy_ctx *ctx, const znippy_rows *r, std::vector<RrRow> &rows, const std::vector<uint32_t> &sel, const void *d_blobs, uint64_t blob_base, int pool,
                           bool verify = false, bool stored = false) {
    // (two names: a call may run both passes, and consumers key the kernel times by name)
    const size_t m = sel.size();
    if (!m) return ZNIPPY_OK;
    std::vector<uint64_t> bo(m), bs(m), us(m), oo(m);
    std::vector<int32_t> st(m, 0);
    std::vector<uint8_t> ck(verify ? 32 * m : 0), dig(verify ? 32 * m : 0), bitmap(stored ? (m + 7) / 8 : 0, 0);
    for (size_t i = 0; i < m; i++) {
        const RrRow &w = rows[sel[i]];
        bo[i] = r->h_blob_off[w.row]; bs[i] = r->h_blob_size[w.row]; us[i] = r->h_len[w.row]; oo[i] = w.slot;
        if (verify) memcpy(&ck[32 * i], &r->h_checksum[(size_t)32 * w.row], 32);
    }
    znippy_rows *t = nullptr;
    int rc = znippy_rows_create(ctx, bo.data(), bs.data(), stored ? bitmap.data() : nullptr, us.data(), stored ? nullptr : oo.data(), verify ? ck.data() : nullptr, 0, m, &t);
    if (rc) return rc;
    const int keep = ctx->n_ktimes, level = ctx->sw.ktime;
    ktime_begin(ctx, stored ? "range_verify_rows" : pool ? "range_decode_rows_late" : "range_decode_rows");
    const bool open = ctx->ktime_open;
    ctx->sw.ktime = 0;  // (the run's own brackets would start the list anew)
    rc = stored ? rows_queue(ctx, t, d_blobs, blob_base, nullptr, 0, true)
                : rows_queue(ctx, t, d_blobs, blob_base, ctx->rr_pool[pool], ctx->rr_cap[pool], false, !verify);
    ctx->sw.ktime = level; ctx->n_ktimes = keep; ctx->ktime_open = open;
    ktime_end(ctx);
    if (!rc) rc = znippy_rows_results(ctx, t, nullptr, nullptr, 0, st.data());
    if (!rc && verify) rc = znippy_rows_digests(ctx, t, dig.data());
    znippy_rows_destroy(t);
    if (rc) return rc;
    for (size_t i = 0; i < m; i++) {
        RrRow &w = rows[sel[i]];
        w.status = st[i];
        if (verify && !st[i]) {
            w.hashed = true;
            if (memcmp(&dig[32 * i], &ck[32 * i], 32)) w.status = ZNIPPY_E_DIGEST;
        }
    }
    return ZNIPPY_OK;
}

// ---- block tree (znippy_rows_block_tree_*, znippy_rows_set_block_tree) ---------------------------------
// Entries of a row: tree_entries_of (host/range_plan.h).
static int rows_tree_layout(znippy_ctx *ctx, znippy_rows *r) {
    const int rc = rows_host_columns(ctx, r);
    if (rc || !r->tree_first.empty()) return rc;
    std::vector<uint64_t> first((size_t)r->shape.n + 1, 0);
    for (uint32_t i = 0; i < r->shape.n; i++) first[i + 1] = first[i] + tree_entries_of(r->h_len[i]);
    r->tree_first.swap(first);
    return ZNIPPY_OK;
}

// One k_block_cvs launch over host-built items, synchronous: write mode (d_out) or compare mode (d_expect, *ok = per item verdict).
static int block_cvs_run(znippy_ctx *ctx, const std::vector<BlockCvItem> &items, uint32_t *d_out, const uint32_t *d_expect, std::vector<uint32_t> *ok, const char *name) {
    if (items.empty()) return ZNIPPY_OK;
    if (items.size() > RR_ITEMS_MAX) return ZNIPPY_E_NOMEM;
    hipStream_t s = ctx->stream;
    SyncFree<BlockCvItem, uint32_t> g{ctx};  // a = the items, b = the verdicts
    const uint32_t n = (uint32_t)items.size();
    if (tmalloc(ctx, &g.a, sizeof(BlockCvItem) * (size_t)n) != hipSuccess || (d_expect && tmalloc(ctx, &g.b, 4 * (size_t)n) != hipSuccess)) return ZNIPPY_E_NOMEM;
    HIPCHK(ctx, hipMemcpyAsync(g.a, items.data(), sizeof(BlockCvItem) * (size_t)n, hipMemcpyHostToDevice, s));
    timed(ctx, name, s, [&] { launch_block_cvs(g.a, n, d_out, d_expect, g.b, s); });
    if (ok) {
        ok->assign(n, 0);
        if (d_expect) HIPCHK(ctx, hipMemcpyAsync(ok->data(), g.b, 4 * (size_t)n, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(ctx, hipStreamSynchronize(s));
    HIPCHK(ctx, hipGetLastError());
    return ZNIPPY_OK;
}

// The entries of the table rows `sel` (in d_tree, laid out by tree_first) folded and compared with the rows' checksums, synchronous:
// ok[i] = the entries of sel[i] are authentic.
static int tree_fold_check(znippy_ctx *ctx, znippy_rows *r, const uint32_t *d_tree, const std::vector<uint32_t> &sel, std::vector<uint32_t> &ok) {
    ok.assign(sel.size(), 0);
    if (sel.empty()) return ZNIPPY_OK;
    hipStream_t s = ctx->stream;
    std::vector<BlockTreeRow> h(sel.size());
    for (size_t i = 0; i < sel.size(); i++) h[i] = BlockTreeRow{r->tree_first[sel[i]], (uint32_t)(r->tree_first[sel[i] + 1] - r->tree_first[sel[i]]), sel[i]};
    SyncFree<BlockTreeRow, uint32_t> g{ctx};  // a = the rows, b = the verdicts
    if (tmalloc(ctx, &g.a, sizeof(BlockTreeRow) * h.size()) != hipSuccess || tmalloc(ctx, &g.b, 4 * h.size()) != hipSuccess) return ZNIPPY_E_NOMEM;
    HIPCHK(ctx, hipMemcpyAsync(g.a, h.data(), sizeof(BlockTreeRow) * h.size(), hipMemcpyHostToDevice, s));
    timed(ctx, "block_tree_fold", s, [&] { launch_block_tree_fold(g.a, (uint32_t)h.size(), d_tree, r->checksum, g.b, s); });
    HIPCHK(ctx, hipMemcpyAsync(ok.data(), g.b, 4 * h.size(), hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    HIPCHK(ctx, hipGetLastError());
    return ZNIPPY_OK;
}

// ---- the range-read call: the plan is host/range_plan.cc, the stages below queue what it describes ----
struct RangeBufs {  // the buffers of one call; every return gives them back
    znippy_ctx *ctx;
    uint8_t *slab = nullptr, *h_slab = nullptr;  // the private columns and lists of the block pass, and their pinned image
    size_t h_cap = 0, up_bytes = 0;
    RangeSlab h{}, d{};
    RangePiece *pieces = nullptr;
    ~RangeBufs() { tfree(ctx, slab); tfree(ctx, pieces); if (h_slab) { (void)hipStreamSynchronize(ctx->stream); pinned_give(ctx, h_slab, h_cap); } }
};

// The slab of the block pass: allocated on both sides, filled on the host.
static int range_slab_make(znippy_ctx *ctx, const RrTable &t, const RangePlan &p, RangeBufs &b) {
    const size_t bytes = range_slab_layout(p, &b.up_bytes);
    if (!(b.h_slab = (uint8_t *)pinned_take(ctx, bytes + 64, &b.h_cap)) || tmalloc(ctx, &b.slab, bytes) != hipSuccess) return ZNIPPY_E_NOMEM;
    if (ensure_decoder_b(ctx)) return ZNIPPY_E_NOMEM;
    range_slab_bind(b.h_slab, p, b.h);
    range_slab_bind(b.slab, p, b.d);
    range_slab_fill(t, p, b.h_slab);
    return ZNIPPY_OK;
}

// The block pass, queued: header scan of the candidate frames, the needed blocks, the rows' verdicts and the decoded total on their way back.
static int run_range_blocks(znippy_ctx *ctx, const RangePlan &p, const RangeBufs &bufs, const void *d_blobs, uint64_t blob_base) {
    hipStream_t s = ctx->stream;
    const RangeSlab &d = bufs.d;
    const uint32_t m = (uint32_t)p.part.size();
    HIPCHK(ctx, hipMemcpyAsync(bufs.slab, bufs.h_slab, bufs.up_bytes, hipMemcpyHostToDevice, s));
    BlockScanArgs b{};
    b.cand_row = d.cand_row; b.cand_base = d.cand_base; b.cand_nblocks = d.cand_nb; b.n_cand = m;
    b.blobs = (const uint8_t *)d_blobs; b.blob_base = blob_base;
    b.blob_off = d.blob_off; b.blob_size = d.blob_size; b.usize = d.usize; b.out_off = d.out_off;
    b.out_cap = ~0ull;  // (the slots fit the scratch by construction)
    b.item_src = d.item_src; b.row_flag = d.row_flag; b.status = d.status;
    timed(ctx, "range_scan", s, [&] { launch_scan_blocks(b, s); });
    DecodeArgs a{};
    a.blobs = b.blobs; a.blob_base = blob_base;
    a.blob_off = d.blob_off; a.blob_size = d.blob_size; a.usize = d.usize; a.out_off = d.out_off;
    a.out = ctx->rr_pool[0]; a.out_cap = ~0ull; a.status = d.status;
    a.block_mode = 1;
    a.item_row = d.item_row; a.item_k = d.item_k; a.item_src = d.item_src; a.n_items = (uint32_t)p.n_items; a.row_flag = d.row_flag;
    a.todo = d.todo; a.n_todo = d.ctl;
    a.pending_count = d.ctl + 2;
    a.compressed = d.comp;
    a.n_rows = m; a.cursor = d.ctl + 1;
    a.lit_scratch = ctx->lit_scratch_b;
    timed(ctx, "range_decode_blocks", s, [&] { launch_decode(a, (int)std::min<uint64_t>((uint64_t)ctx->decode_grid, p.n_todo), false, s); });
    launch_range_status(d.row_flag, d.block_bytes, m, d.late, d.decoded, s);
    HIPCHK(ctx, hipMemcpyAsync(bufs.h.late, d.late, m, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(bufs.h.decoded, d.decoded, 8, hipMemcpyDeviceToHost, s));
    return ZNIPPY_OK;
}

// Verified: every block that will serve a range — decoded into the scratch, or a stored row's where it lies — is hashed on its own
// and compared with its (accepted) entry, before a byte of it moves.
static int run_range_verify_blocks(znippy_ctx *ctx, const znippy_rows *r, const RrTable &t, RangePlan &p, const void *d_blobs, uint64_t blob_base, uint64_t *hashed) {
    std::vector<BlockCvItem> items;
    std::vector<std::pair<uint32_t, uint32_t>> item_of;
    *hashed = range_plan_block_items(t, p, ctx->rr_pool[0], (const uint8_t *)d_blobs, blob_base, items, item_of);
    if (items.empty()) return ZNIPPY_OK;
    std::vector<uint32_t> ok;
    const int rc = block_cvs_run(ctx, items, nullptr, r->tree_dev, &ok, "range_verify_blocks");
    if (rc) return rc;
    for (size_t j = 0; j < items.size(); j++)
        if (!ok[j]) p.rows[item_of[j].first].bad[item_of[j].second] = 1;
    return ZNIPPY_OK;
}

// The gather: every piece from where its bytes are to its place in d_out, synchronous.
static int run_range_gather(znippy_ctx *ctx, const std::vector<RangePiece> &pieces, RangeBufs &bufs) {
    if (pieces.empty()) return ZNIPPY_OK;
    hipStream_t s = ctx->stream;
    if (tmalloc(ctx, &bufs.pieces, sizeof(RangePiece) * pieces.size()) != hipSuccess) return ZNIPPY_E_NOMEM;
    HIPCHK(ctx, hipMemcpy(bufs.pieces, pieces.data(), sizeof(RangePiece) * pieces.size(), hipMemcpyHostToDevice));
    timed(ctx, "range_copy", s, [&] {
        for (size_t at = 0; at < pieces.size(); at += (1u << 30)) launch_range_gather(bufs.pieces + at, (uint32_t)std::min<size_t>(pieces.size() - at, 1u << 30), s);
    });
    HIPCHK(ctx, hipStreamSynchronize(s));
    HIPCHK(ctx, hipGetLastError());
    return ZNIPPY_OK;
}

static int rows_read_ranges(znippy_ctx *ctx, znippy_rows *r, const void *d_blobs, uint64_t blob_base, const uint64_t *range_row,
                            const uint64_t *range_begin, const uint64_t *range_len, const uint64_t *range_out, uint64_t n_ranges, void *d_out,
                            uint64_t out_cap, int32_t *range_status, uint64_t *decoded_bytes, bool verified = false, uint64_t *hashed_bytes = nullptr) {
    if (!ctx_enter(ctx)) return ZNIPPY_E_INVAL;
    if (!ctx || !r || r->ctx != ctx) return ZNIPPY_E_INVAL;
    if (verified && !r->checksum && r->shape.n) return ZNIPPY_E_INVAL;  // nothing to verify against
    if (decoded_bytes) *decoded_bytes = 0;
    if (hashed_bytes) *hashed_bytes = 0;
    if (!n_ranges) return ZNIPPY_OK;
    if (!range_row || !range_begin || !range_len || !d_blobs || !d_out) return ZNIPPY_E_INVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = rows_host_columns(ctx, r);
    if (!rc && verified) rc = rows_host_checksum(ctx, r);
    if (rc) return rc;
    ctx->n_ktimes = 0;
    { const int prc = poison_enter(ctx); if (prc) return prc; }
    const PoisonHold hold(ctx);  // (the private runs below decode into the range scratch beside what the block pass left there)

    // the plan: every range validated, the distinct rows, their routes and slots — then the scratch and the block pass's slab
    const RrTable t = rows_table_view(r);
    const RrCall call{range_row, range_begin, range_len, range_out, n_ranges, out_cap, blob_base, verified};
    RangePlan p;
    if ((rc = range_plan_build(t, call, p))) return rc;
    if ((rc = ensure_range_scratch(ctx, 0, p.need0))) return rc;
    const bool blocks = !p.part.empty();
    RangeBufs bufs{ctx};
    if (blocks && (rc = range_slab_make(ctx, t, p, bufs))) return rc;

    // the block pass and, behind it, the rows known from the start to need a whole decode (its results call waits for both)
    if (blocks && (rc = run_range_blocks(ctx, p, bufs, d_blobs, blob_base))) return rc;
    if ((rc = rr_decode_whole(ctx, r, p.rows, p.whole, d_blobs, blob_base, 0, verified))) return rc;
    if ((rc = rr_decode_whole(ctx, r, p.rows, p.stored_whole, d_blobs, blob_base, 0, true, true))) return rc;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipGetLastError());

    // what the block pass gave up on — a frame the scan does not vouch for, a block that needs history — is decoded whole
    if (blocks) {
        std::vector<uint32_t> late;
        uint64_t need1 = 0;
        if ((rc = range_plan_late(t, p, bufs.h.late, late, need1))) return rc;
        if ((rc = ensure_range_scratch(ctx, 1, need1))) return rc;  // (nothing is queued at this point, and d_out is untouched)
        if ((rc = rr_decode_whole(ctx, r, p.rows, late, d_blobs, blob_base, 1, verified))) return rc;
    }
    uint64_t hashed = 0;
    if (verified && (rc = run_range_verify_blocks(ctx, r, t, p, d_blobs, blob_base, &hashed))) return rc;

    // the gather: every good range from where its bytes are to its place in d_out
    const uint8_t *const pools[2] = {ctx->rr_pool[0], ctx->rr_pool[1]};
    std::vector<RangePiece> pieces;
    range_plan_pieces(t, call, p, pools, (const uint8_t *)d_blobs, (uint8_t *)d_out, pieces);
    if ((rc = run_range_gather(ctx, pieces, bufs))) return rc;
    if (range_status) memcpy(range_status, p.st.data(), 4 * (size_t)n_ranges);
    if (decoded_bytes) *decoded_bytes = range_plan_decoded(t, p, blocks ? *bufs.h.decoded : 0);
    if (hashed_bytes) *hashed_bytes = hashed;
    return ZNIPPY_OK;
}

int znippy_rows_read_ranges(znippy_ctx *ctx, znippy_rows *r, const void *d_blobs, uint64_t blob_base, const uint64_t *range_row,
                            const uint64_t *range_begin, const uint64_t *range_len, const uint64_t *range_out, uint64_t n_ranges, void *d_out,
                            uint64_t out_cap, int32_t *range_status, uint64_t *decoded_bytes) {
    ZN_NO_THROW(rows_read_ranges(ctx, r, d_blobs, blob_base, range_row, range_begin, range_len, range_out, n_ranges, d_out, out_cap, range_status, decoded_bytes))
}

int znippy_rows_read_ranges_verified(znippy_ctx *ctx, znippy_rows *r, const void *d_blobs, uint64_t blob_base, const uint64_t *range_row,
                                     const uint64_t *range_begin, const uint64_t *range_len, const uint64_t *range_out, uint64_t n_ranges, void *d_out,
                                     uint64_t out_cap, int32_t *range_status, uint64_t *decoded_bytes, uint64_t *hashed_bytes) {
    ZN_NO_THROW(rows_read_ranges(ctx, r, d_blobs, blob_base, range_row, range_begin, range_len, range_out, n_ranges, d_out, out_cap, range_status, decoded_bytes,
                                 true, hashed_bytes))
}

static int rows_block_tree_layout(znippy_ctx *ctx, znippy_rows *r, uint64_t *n_entries, uint64_t *row_first) {
    if (!ctx_enter(ctx)) return ZNIPPY_E_INVAL;
    if (!ctx || !r || r->ctx != ctx || !n_entries) return ZNIPPY_E_INVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int rc = rows_tree_layout(ctx, r);
    if (rc) return rc;
    *n_entries = r->tree_first[r->shape.n];
    if (row_first) memcpy(row_first, r->tree_first.data(), 8 * ((size_t)r->shape.n + 1));
    return ZNIPPY_OK;
}

// The producer: every row with entries decoded whole into the range scratch (stored rows: hashed where they lie), one k_block_cvs
// launch in write mode for all of them, then the fold against the checksums.  Not a run, and nothing is installed.
static int rows_block_tree_build(znippy_ctx *ctx, znippy_rows *r, const void *d_blobs, uint64_t blob_base, uint8_t *tree, int32_t *row_status) {
    if (!ctx_enter(ctx)) return ZNIPPY_E_INVAL;
    if (!ctx || !r || r->ctx != ctx) return ZNIPPY_E_INVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = rows_tree_layout(ctx, r);
    if (rc) return rc;
    const uint64_t n_entries = r->tree_first[r->shape.n];
    if (n_entries && (!d_blobs || !tree)) return ZNIPPY_E_INVAL;
    std::vector<int32_t> st(r->shape.n, 0);
    if (row_status && r->shape.n) memset(row_status, 0, 4 * (size_t)r->shape.n);
    if (!n_entries) return ZNIPPY_OK;
    hipStream_t s = ctx->stream;
    ctx->n_ktimes = 0;
    { const int prc = poison_enter(ctx); if (prc) return prc; }
    const PoisonHold hold(ctx);

    // 1) the rows with entries against the blob region; a slot in the scratch for every compressed one — sized before anything is queued
    const RrTable t = rows_table_view(r);
    std::vector<RrRow> rows;
    std::vector<uint32_t> sel;
    uint64_t need0 = 0;
    if ((rc = tree_plan_rows(t, blob_base, st, rows, sel, need0))) return rc;
    if ((rc = ensure_range_scratch(ctx, 0, need0))) return rc;

    // 2) a private decode-only run of the compressed rows
    if ((rc = rr_decode_whole(ctx, r, rows, sel, d_blobs, blob_base, 0))) return rc;
    HIPCHK(ctx, hipStreamSynchronize(s));
    HIPCHK(ctx, hipGetLastError());

    // 3) every block of every good row: one launch
    std::vector<BlockCvItem> items;
    std::vector<uint32_t> good;
    tree_plan_items(t, rows, ctx->rr_pool[0], (const uint8_t *)d_blobs, blob_base, st, good, items);
    SyncFree<uint32_t> g{ctx};  // a = the tree on the device
    if (tmalloc(ctx, &g.a, 32 * (size_t)n_entries) != hipSuccess) return ZNIPPY_E_NOMEM;
    HIPCHK(ctx, hipMemsetAsync(g.a, 0, 32 * (size_t)n_entries, s));
    if ((rc = block_cvs_run(ctx, items, g.a, nullptr, nullptr, "block_tree_cvs"))) return rc;

    // 4) the entries against the checksums (a table without the column compares nothing)
    if (r->checksum) {
        std::vector<uint32_t> ok;
        if ((rc = tree_fold_check(ctx, r, g.a, good, ok))) return rc;
        for (size_t i = 0; i < good.size(); i++)
            if (!ok[i]) st[good[i]] = ZNIPPY_E_DIGEST;
    }
    HIPCHK(ctx, hipMemcpyAsync(tree, g.a, 32 * (size_t)n_entries, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    for (uint32_t ri = 0; ri < r->shape.n; ri++)  // a row that failed has no entries to offer
        if (st[ri]) memset(tree + 32 * r->tree_first[ri], 0, 32 * (size_t)(r->tree_first[ri + 1] - r->tree_first[ri]));
    if (row_status) memcpy(row_status, st.data(), 4 * (size_t)r->shape.n);
    return ZNIPPY_OK;
}

// The installer: the caller's entries go to the device, every row's are folded against its checksum, and only those that match count
// from then on (tree_accept).  The checksum column alone is trusted.
static int rows_set_block_tree(znippy_ctx *ctx, znippy_rows *r, const uint8_t *tree, int32_t *row_status) {
    if (!ctx_enter(ctx)) return ZNIPPY_E_INVAL;
    if (!ctx || !r || r->ctx != ctx) return ZNIPPY_E_INVAL;
    if (!r->checksum) return ZNIPPY_E_INVAL;  // nothing could authenticate the entries
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    if (row_status && r->shape.n) memset(row_status, 0, 4 * (size_t)r->shape.n);
    if (!tree) {
        HIPCHK(ctx, hipStreamSynchronize(s));
        tfree(ctx, r->tree_dev);
        r->tree_dev = nullptr;
        r->tree_accept.clear();
        return ZNIPPY_OK;
    }
    int rc = rows_tree_layout(ctx, r);
    if (rc) return rc;
    const uint64_t n_entries = r->tree_first[r->shape.n];
    ctx->n_ktimes = 0;
    SyncFree<uint32_t> g{ctx};  // a = the tree on the device
    std::vector<uint8_t> accept(r->shape.n, 0);
    if (n_entries) {
        if (tmalloc(ctx, &g.a, 32 * (size_t)n_entries) != hipSuccess) return ZNIPPY_E_NOMEM;
        HIPCHK(ctx, hipMemcpyAsync(g.a, tree, 32 * (size_t)n_entries, hipMemcpyHostToDevice, s));
        std::vector<uint32_t> sel, ok;
        for (uint32_t ri = 0; ri < r->shape.n; ri++)
            if (r->tree_first[ri + 1] != r->tree_first[ri]) sel.push_back(ri);
        if ((rc = tree_fold_check(ctx, r, g.a, sel, ok))) return rc;
        for (size_t i = 0; i < sel.size(); i++) {
            accept[sel[i]] = ok[i] ? 1 : 0;
            if (!ok[i] && row_status) row_status[sel[i]] = ZNIPPY_E_DIGEST;
        }
    }
    HIPCHK(ctx, hipStreamSynchronize(s));
    std::swap(r->tree_dev, g.a);  // (the guard frees the tree this one replaces)
    r->tree_accept.swap(accept);
    return ZNIPPY_OK;
}

int znippy_rows_block_tree_layout(znippy_ctx *ctx, znippy_rows *r, uint64_t *n_entries, uint64_t *row_first) { ZN_NO_THROW(rows_block_tree_layout(ctx, r, n_entries, row_first)) }
int znippy_rows_block_tree_build(znippy_ctx *ctx, znippy_rows *r, const void *d_blobs, uint64_t blob_base, uint8_t *tree, int32_t *row_status) {
    ZN_NO_THROW(rows_block_tree_build(ctx, r, d_blobs, blob_base, tree, row_status))
}
int znippy_rows_set_block_tree(znippy_ctx *ctx, znippy_rows *r, const uint8_t *tree, int32_t *row_status) { ZN_NO_THROW(rows_set_block_tree(ctx, r, tree, row_status)) }

int znippy_rows_digests(znippy_ctx *ctx, znippy_rows *r, uint8_t *digests) {
    if (!ctx_enter(ctx)) return ZNIPPY_E_INVAL;
    if (!ctx || !r || !digests) return ZNIPPY_E_INVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (r->lane_used) HIPCHK(ctx, lanes_sync(ctx));
    if (r->aux_used) HIPCHK(ctx, hipStreamSynchronize(ctx->aux));  // the latest run's verify may be queued there
    if (r->shape.n && r->run_seq) { const int rc = rows_settle(ctx, r, (unsigned)((r->run_seq - 1) & 1)); if (rc) return rc; }
    if (r->run_seq && r->run_args[(r->run_seq - 1) & 1].plain) return ZNIPPY_E_INVAL;  // a decode-only run computes no digest
    if (r->shape.n) HIPCHK(ctx, hipMemcpy(digests, r->digests, 32 * (size_t)r->shape.n, hipMemcpyDeviceToHost));
    return ZNIPPY_OK;
}

// ---- rounds -------------------------------------------------------------------------------------
void znippy_rounds_destroy(znippy_rounds *r) {
    if (!r) return;
    (void)hipSetDevice(r->ctx->device);
    if (r->ctx->copy) (void)hipStreamSynchronize(r->ctx->copy);  // a result copy may still be reading a slab
    for (int k = 0; k < 2; k++) {
        pinned_give(r->ctx, r->h_res_m[k], r->h_res_cap_m[k]);
        event_give(r->ctx, r->ev_enc[k]);
        event_give(r->ctx, r->ev_res[k]);
        pinned_give(r->ctx, r->h_tree_m[k], r->h_tree_cap_m[k]);
        tfree(r->ctx, r->tree_m[k]);
    }
    tfree(r->ctx, r->tree_units);
    void *ptrs[] = {r->src_off, r->len, r->skip, r->res_m[0], r->res_m[1], r->items, r->piece_len, r->piece_len_init,
                    r->piece_start, r->local_excl, r->block_tot, r->first_item, r->piece_pad, r->stored, r->order_small, r->order_wide, r->retry_list, r->retry_count,
                    r->plan_scratch[0], r->plan_scratch[1], r->plan_scratch[2], r->d_ldm, r->d_ldm_desc};
    pinned_give(r->ctx, r->h_stored, r->h_stored_cap);
    for (void *p : ptrs)
        tfree(r->ctx, p);
    free_plan(r->ctx, r->plan);
    znippy_ctx *const c = r->ctx;
    delete r;
    table_released(c);
}

// The stages of znippy_rounds_create, in its order.  Every failure returns; the constructor's scope guard frees what was made.
static int rounds_columns_h2d(znippy_ctx *ctx, znippy_rounds *r, const uint64_t *src_offset, const uint64_t *len, const uint8_t *skip) {
    const size_t n = r->n;
    int rc;
    if ((rc = dev_upload(ctx, &r->src_off, src_offset, n)) || (rc = dev_upload(ctx, &r->len, len, n)) ||
        (skip ? (rc = dev_upload(ctx, &r->skip, skip, n)) : (tmalloc(ctx, &r->skip, std::max<size_t>(n, 16)) != hipSuccess ? (rc = ZNIPPY_E_NOMEM) : 0)))
        return rc;
    if (!skip && n) HIPCHK(ctx, hipMemsetAsync(r->skip, 0, n, ctx->stream));
    return ZNIPPY_OK;
}

static int rounds_slabs(znippy_ctx *ctx, znippy_rounds *r) {
    r->res_bytes = ResSlab::bytes(r->n);
    for (int k = 0; k < 2; k++)
        if (tmalloc(ctx, &r->res_m[k], r->res_bytes) != hipSuccess ||
            !(r->h_res_m[k] = (uint8_t *)pinned_take(ctx, r->res_bytes, &r->h_res_cap_m[k])) ||
            !(r->ev_enc[k] = event_take(ctx)) || !(r->ev_res[k] = event_take(ctx)))
            return ZNIPPY_E_NOMEM;
    return ZNIPPY_OK;
}

static int rounds_hash_plan(znippy_ctx *ctx, znippy_rounds *r, const uint64_t *len) {
    const uint32_t n = r->n;
    PlanBuf p;
    build_plan([&](uint32_t u) { return len[u]; }, n, p);
    const int rc = upload_plan(ctx, p, r->plan);
    if (rc) return rc;
    if (r->n_items == n && r->n_wide == 0 && r->enc_bytes == r->in_bytes && n) {
        uint32_t max_units = 0;
        for (const Tile &t : p.tiles) max_units = std::max(max_units, t.n_units);
        r->fuse_tiles = 1;  // one tile per dequeue (C2: 6 rounds): 0.77 ms against 0.86 for two and 1.12 for ten on one box — with ~4 tiles per wave the finest grain balances best
        if (const char *e = getenv("ZNIPPY_FUSE_TILES")) { const int v = atoi(e); if (v >= 1 && v * (int)max_units <= 64) r->fuse_tiles = v; }  // A/B
    }
    return ZNIPPY_OK;
}

// far window: regions of the index for the encoded rounds longer than one block (rounds of 4 GiB and more are not
// indexed: the index holds 32-bit positions).  Every round has at least one piece: with no more pieces than rounds
// there is no such round, and the pass is skipped (100k small rounds: no host pass of its own)
static void rounds_far_regions(znippy_rounds *r, const uint64_t *len, const uint8_t *skip) {
    const uint64_t n = r->n;
    if (r->n_items > n) {
        for (uint64_t i = 0; i < n; i++)
            if (len[i] > BLOCK_BYTES && len[i] < (1ull << 32) && !(skip && skip[i])) {
                const uint32_t lg = ldm_log2(len[i]);
                r->h_ldm.push_back(LdmRound{(uint32_t)i, r->ldm_chunks, r->ldm_entries | ((uint64_t)lg << 48)});
                r->ldm_entries += 1ull << lg;
                r->ldm_chunks += (uint32_t)((len[i] + LDM_CHUNK - 1) / LDM_CHUNK);
            }
    }
}

// encoder plan: one item per output piece, in round order — counted, scanned and filled on the device
static int rounds_encoder_plan(znippy_ctx *ctx, znippy_rounds *r, bool has_skip) {
    const size_t n = r->n, ni = std::max<size_t>(r->n_items, 1), nsb = (ni + 255) / 256;
    const uint32_t nblk = ((uint32_t)n + 1023) / 1024;
    RoundSums *sums = nullptr;
    auto take = [&](auto **p, size_t bytes) { return tmalloc(ctx, p, bytes) == hipSuccess; };  // (at least 16 bytes each)
    const bool ok = take(&r->first_item, 4 * n) && take(&sums, std::max<size_t>(sizeof(RoundSums) * (size_t)nblk, 64)) &&
                    take(&r->order_small, 4 * (size_t)r->n_small) && take(&r->order_wide, 4 * (size_t)r->n_wide) &&
                    take(&r->retry_list, 4 * (size_t)r->n_small) && take(&r->retry_count, 64) && take(&r->stored, n) &&
                    (r->h_stored = (uint8_t *)pinned_take(ctx, std::max<size_t>(n, 16), &r->h_stored_cap)) != nullptr &&
                    take(&r->items, sizeof(EncItem) * ni) && take(&r->piece_len_init, 4 * ni) && take(&r->piece_len, 4 * ni) &&
                    take(&r->piece_start, 8 * ni) && take(&r->local_excl, 8 * ni) && take(&r->block_tot, 8 * nsb);
    r->plan_scratch[0] = sums;  // (parked until the table goes: the kernels below are still queued then)
    if (!ok) return ZNIPPY_E_NOMEM;
    if (n) {
        const uint8_t *const d_skip = has_skip ? r->skip : (const uint8_t *)nullptr;
        hipLaunchKernelGGL(k_rounds_sums, dim3(nblk), dim3(256), 0, ctx->stream, r->len, d_skip, (uint32_t)n, sums);
        hipLaunchKernelGGL(k_rounds_scan, dim3(1), dim3(256), 0, ctx->stream, sums, nblk);
        hipLaunchKernelGGL(k_rounds_fill, dim3(nblk), dim3(256), 0, ctx->stream, r->len, d_skip, (uint32_t)n, sums, r->first_item, r->items, r->piece_len_init,
                           r->order_small, r->order_wide);
    }
    return ZNIPPY_OK;
}

int znippy_rounds_create(znippy_ctx *ctx, const uint64_t *src_offset, const uint64_t *len,
                         const uint8_t *skip, uint64_t n, znippy_rounds **out) {
    if (!ctx_enter(ctx)) return ZNIPPY_E_INVAL;
    if (!ctx || !out || (n && (!src_offset || !len)) || n >= 0xFFFFFFF0ull) return ZNIPPY_E_INVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    TDbg td(ctx->sw.tdbg, "rounds_create");
    std::unique_ptr<znippy_rounds, void (*)(znippy_rounds *)> guard(new znippy_rounds(), znippy_rounds_destroy);  // every failure below: return
    znippy_rounds *const r = guard.get();
    r->ctx = ctx;
    ctx->live_tables++;
    r->n = (uint32_t)n;
    if (skip) r->h_skip.assign(skip, skip + n);  // (results: which rounds are stored; empty = none)
    uint64_t tot[8];
    zn_rounds_totals(len, skip, n, tot);  // sizes of the device arrays; the arrays themselves are filled on the device
    r->blob_bound = tot[4]; r->in_bytes = tot[5]; r->enc_bytes = tot[6];
    r->all_stored_aligned = n > 0 && r->enc_bytes == 0 && !tot[7];
    if (tot[0] >= 0xFFFFFFF0ull) return ZNIPPY_E_INVAL;
    r->n_items = (uint32_t)tot[0]; r->prov_bytes = tot[1]; r->n_small = (uint32_t)tot[2]; r->n_wide = (uint32_t)tot[3];
    td.mark("totals");
    int rc;
    if ((rc = rounds_columns_h2d(ctx, r, src_offset, len, skip))) return rc;
    td.mark("columns_h2d");
    if ((rc = rounds_slabs(ctx, r))) return rc;
    td.mark("slabs");
    if ((rc = rounds_hash_plan(ctx, r, len))) return rc;
    td.mark("hash_plan");
    rounds_far_regions(r, len, skip);
    if ((rc = rounds_encoder_plan(ctx, r, skip != nullptr))) return rc;
    td.mark("encoder_plan");
    // store-path pieces keep their fixed lengths for the table's lifetime; encoded pieces are rewritten by
    // the encoder on every run, so one copy at creation is enough
    if (r->n_items) HIPCHK(ctx, hipMemcpyAsync(r->piece_len, r->piece_len_init, 4 * (size_t)r->n_items, hipMemcpyDeviceToDevice, ctx->stream));
    td.mark("rest");
    *out = guard.release();
    return ZNIPPY_OK;
}

// (aligned blob offsets: in front of every round but the first, at most align - 1 bytes of gap)
uint64_t znippy_rounds_blob_bound(const znippy_rounds *r) {
    if (!r) return 0;
    return r->blob_bound + (r->n ? (uint64_t)(r->n - 1) * (r->blob_align - 1) : 0);
}

// the rounds as hash input, digests into `res` (the hash kernel's arguments, and the encoder's where its waves hash: EncodeArgs::h)
static HashArgs rounds_hash_args(const znippy_rounds *r, const ResSlab &res, const void *d_src) {
    HashArgs h{};
    h.tiles = r->plan.tiles; h.n_tiles = r->plan.n_tiles;
    h.len = r->len;
    h.srcA = (const uint8_t *)d_src; h.offA = r->src_off; h.baseA = 0;
    h.digests = res.digests(); h.tile_cv = r->plan.tile_cv;
    return h;
}
// res: the slab the digests go to (and whose blob offsets a copying launch reads)
// d_copy_out != nullptr: the stored (skip) rounds are copied to d_copy_out + blob_offset[round] while they are hashed
// (store-heavy tables; blob_offset must have been computed on the stream before)
// copy_align: the alignment of the run's blob offsets (16 and more: every destination is as aligned as d_copy_out is)
// tree_out != nullptr: the run's block tree entries (znippy_rounds_emit_block_tree), made from the tile CVs behind the merge
static int hash_rounds_async(znippy_ctx *ctx, znippy_rounds *r, const ResSlab &res, const void *d_src, hipStream_t on = nullptr,
                             void *d_copy_out = nullptr, uint64_t copy_cap = 0, uint32_t copy_align = 1, uint32_t *tree_out = nullptr) {
    hipStream_t s = on ? on : ctx->stream;
    HashArgs h = rounds_hash_args(r, res, d_src);
    if (d_copy_out) {
        h.srcB = (uint8_t *)d_copy_out; h.offB = res.blob_offset(); h.copy_to_B = 1;
        h.store_tiles = ctx->sw.store_g;
        h.copy_mask = r->skip; h.copy_cap = copy_cap;
        h.misaligned_dst = !((r->all_stored_aligned || copy_align >= 16) && ((uintptr_t)d_copy_out & 15) == 0);
    }
    // next to a busy encoder (auxiliary stream) the hash keeps out of LDS: the encoder's residency depends on it
    if (on && r->enc_bytes * 4 >= r->in_bytes) h.fold_tiles_max = 1;
    timed(ctx, "blake3_tiles", s, [&] { launch_hash_tiles(h, s); });
    if (r->plan.n_big) {
        // beside the persistent encoder (auxiliary stream) the merge stays with its one-wave workgroups: a four-wave one waits for
        // four free wave slots on one CU, which the encoder's waves leave only when they retire (seen: 53 ms behind a 65 ms encode)
        timed(ctx, "blake3_merge_big", s, [&] {
            launch_merge_big(r->plan.big, r->plan.n_big, r->plan.tile_cv, res.digests(), r->plan.grp_big, r->plan.grp_k, r->plan.n_grp, on ? 0xFFFFFFFFu : r->plan.max_cvs, s);
        });
        // same stream, directly behind the merge: whatever orders the merge (ev_join, the main stream) orders this too, and the
        // next run's hash, which overwrites tile_cv, is behind it as it is behind the merge
        if (tree_out)
            timed(ctx, "block_tree_entries", s, [&] { launch_round_block_entries(r->tree_units, r->n_tree_units, r->n_tree_entries, r->plan.tile_cv, tree_out, s); });
    }
    HIPCHK(ctx, hipGetLastError());
    return ZNIPPY_OK;
}

int znippy_hash_rounds(znippy_ctx *ctx, znippy_rounds *r, const void *d_src, uint8_t *digests) {
    if (!ctx_enter(ctx)) return ZNIPPY_E_INVAL;
    if (!ctx || !r || r->ctx != ctx || !digests || (r->n && !d_src)) return ZNIPPY_E_INVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ctx->n_ktimes = 0;
    { const int prc = poison_enter(ctx); if (prc) return prc; }
    const ResSlab res = r->dev(r->slot);
    int rc = hash_rounds_async(ctx, r, res, d_src);
    if (rc) return rc;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (r->n) HIPCHK(ctx, hipMemcpy(digests, res.digests(), 32 * (size_t)r->n, hipMemcpyDeviceToHost));
    return ZNIPPY_OK;
}

// ---- single-chunk shims -------------------------------------------------------------------------
static int shim_reserve(znippy_ctx *ctx, size_t in_need, size_t out_need) {
    if (in_need > ctx->shim_in_cap || !ctx->shim_in) {
        if (ctx->shim_in) (void)hipFree(ctx->shim_in);
        ctx->shim_in = nullptr; ctx->shim_in_cap = 0;
        size_t cap = std::max<size_t>(in_need + 64, 1 << 16);
        HIPCHK(ctx, hipMalloc(&ctx->shim_in, cap));
        ctx->shim_in_cap = cap;
        if (ctx->sw.poison) HIPCHK(ctx, poison_dev(ctx, ctx->shim_in, cap));
    }
    if (out_need > ctx->shim_out_cap || !ctx->shim_out) {
        if (ctx->shim_out) (void)hipFree(ctx->shim_out);
        ctx->shim_out = nullptr; ctx->shim_out_cap = 0;
        size_t cap = std::max<size_t>(out_need + 64, 1 << 16);
        HIPCHK(ctx, hipMalloc(&ctx->shim_out, cap));
        ctx->shim_out_cap = cap;
        if (ctx->sw.poison) HIPCHK(ctx, poison_dev(ctx, ctx->shim_out, cap));
    }
    return ZNIPPY_OK;
}

int znippy_blake3(znippy_ctx *ctx, const void *src, size_t n, uint8_t out[32]) {
    if (!ctx_enter(ctx)) return ZNIPPY_E_INVAL;
    if (!ctx || !out || (n && !src)) return ZNIPPY_E_INVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = shim_reserve(ctx, n, 0);
    if (rc) return rc;
    if (n) HIPCHK(ctx, hipMemcpyAsync(ctx->shim_in, src, n, hipMemcpyHostToDevice, ctx->stream));
    uint64_t off = 0, len = n;
    znippy_rounds *r = nullptr;
    rc = znippy_rounds_create(ctx, &off, &len, nullptr, 1, &r);
    if (rc) return rc;
    rc = znippy_hash_rounds(ctx, r, ctx->shim_in, out);
    znippy_rounds_destroy(r);
    return rc;
}

int znippy_decompress(znippy_ctx *ctx, const void *frame, size_t n, void *dst, size_t cap, size_t *written) {
    if (!ctx_enter(ctx)) return ZNIPPY_E_INVAL;
    if (!ctx || !frame || !written || (cap && !dst)) return ZNIPPY_E_INVAL;
    uint64_t usize = 0;
    int rc = znippy_get_decompressed_size(frame, n, &usize);
    if (rc) return rc;
    {  // the kernels want the Zstandard magic at byte 0: leading skippable frames stay on the host
        const ptrdiff_t skip = skippable_prefix((const uint8_t *)frame, n);
        frame = (const uint8_t *)frame + skip;
        n -= (size_t)skip;
    }
    if (usize > cap) return ZNIPPY_E_DST_SMALL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    rc = shim_reserve(ctx, n, usize);
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(ctx->shim_in, frame, n, hipMemcpyHostToDevice, ctx->stream));
    uint64_t boff = 0, bsz = n, ooff = 0;
    znippy_rows *r = nullptr;
    rc = znippy_rows_create(ctx, &boff, &bsz, nullptr, &usize, &ooff, nullptr, 0, 1, &r);
    if (rc) return rc;
    int32_t status = 0;
    rc = znippy_decode_verify_rows(ctx, r, ctx->shim_in, 0, ctx->shim_out, ctx->shim_out_cap, nullptr, nullptr, 0, &status);
    znippy_rows_destroy(r);
    if (rc) return rc;
    if (status) return status;
    if (usize) HIPCHK(ctx, hipMemcpy(dst, ctx->shim_out, usize, hipMemcpyDeviceToHost));
    *written = usize;
    return ZNIPPY_OK;
}

}  // extern "C"


// A run's results (offsets, sizes, digests: 48 bytes per round) leave through this kernel, written straight into the
// slot's pinned host mirror (device-visible: hipHostMalloc).  hipMemcpyAsync did the same with a blit kernel of its own,
// but the CALL blocked 6.7-7.4 ms once per table — in the third run, whatever had been copied before (time marks around
// every HIP call of that run: everything else 0.06 ms together; tools/write_steps.py) — which put one 7-12 ms step among
// bench.py's 0.8 ms write steps, behind its three warm-up steps: a quarter of the write leg's rate.  A launch has no such
// mode.
__global__ __launch_bounds__(256) void k_results_out(uint4 *dst, const uint4 *src, uint32_t n16) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n16; i += gridDim.x * 256) dst[i] = src[i];
}

// ---- write side ------------------------------------------------------------------------------------
// Far window of a windowed encode call: the context's index (grow-only) and the table's region list and per-round
// descriptors (once per table).  Any failure leaves the far window off for the call — the near window still works.
static bool ensure_ldm(znippy_ctx *ctx, znippy_rounds *r) {
    if (!r->ldm_entries || r->ldm_entries > LDM_MAX_ENTRIES) return false;
    if (r->ldm_entries > ctx->ldm_cap) {
        if (ctx->ldm) {
            if (hipStreamSynchronize(ctx->stream) != hipSuccess) return false;  // an earlier call may still read it
            (void)hipFree(ctx->ldm);
        }
        ctx->ldm = nullptr; ctx->ldm_cap = 0;
        if (hipMalloc(&ctx->ldm, 4 * r->ldm_entries) != hipSuccess) { (void)hipGetLastError(); ctx->ldm = nullptr; return false; }
        ctx->ldm_cap = r->ldm_entries;
        if (ctx->sw.poison) (void)poison_dev(ctx, ctx->ldm, 4 * r->ldm_entries);
    }
    if (!r->d_ldm) {
        std::vector<uint64_t> desc(r->n, LDM_NONE);
        for (const LdmRound &e : r->h_ldm) desc[e.round] = e.desc;
        LdmRound *dl = nullptr;
        uint64_t *dd = nullptr;
        if (tmalloc(ctx, &dl, sizeof(LdmRound) * r->h_ldm.size()) != hipSuccess || tmalloc(ctx, &dd, 8 * (size_t)r->n) != hipSuccess ||
            hipMemcpy(dl, r->h_ldm.data(), sizeof(LdmRound) * r->h_ldm.size(), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(dd, desc.data(), 8 * (size_t)r->n, hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipGetLastError();
            tfree(ctx, dl);
            tfree(ctx, dd);
            return false;
        }
        r->d_ldm = dl; r->d_ldm_desc = dd;
    }
    return true;
}

// ---- one run of a rounds table: the plan (host/enc_plan.cc), then the stages in the order rounds_launch queues them ----------
// what the caller gave a run, and what of the table is the run's own: its slot's slab and tree buffer, the alignment it was queued with
struct EncRun { const void *d_src; void *d_blob_out; uint64_t blob_cap; unsigned slot; ResSlab res; uint32_t *tree_out; uint32_t align; const uint32_t *pad; };
static_assert(ENC_HIGH_TIER_LEVEL == HIGH_TIER_LEVEL, "host/enc_plan.h restates the tier boundary of encode.h");

static EncShape rounds_shape(const znippy_rounds *r) {
    return EncShape{r->n, r->n_items, r->n_small, r->n_wide, r->in_bytes, r->enc_bytes, r->fuse_tiles, r->plan.n_tiles, r->n_tree_entries, r->ldm_entries,
                    r->store_incompressible, r->emit_tree, r->blob_align};
}
static EncodeArgs rounds_encode_args(znippy_ctx *ctx, const znippy_rounds *r, const EncPlan &p, const EncRun &run) {
    EncodeArgs a{};
    a.items = r->items;
    a.src = (const uint8_t *)run.d_src; a.src_off = r->src_off; a.len = r->len;
    a.prov = ctx->enc_prov; a.seq_scratch = ctx->enc_seq;
    a.piece_len = r->piece_len; a.piece_start = r->piece_start; a.tabs = ctx->enc_tabs;
    a.high = p.high;
    a.tail_mark = p.tail_mark;
    a.window_log = p.window_log;
    if (p.far) { a.ldm = ctx->ldm; a.ldm_desc = r->d_ldm_desc; }
    if (ctx->sw.edbg)  // diagnostic: phase shares of the previous run's wide-variant blocks
        a.dbg = diag_cycle<8>(ctx, znippy_ctx::DIAG_ENCODE, ctx->stream, nullptr, [](const unsigned long long *h) {
            if (h[0]) fprintf(stderr, "[znippy edbg] wide blocks=%llu  cycles per block: setup=%.0f matching=%.0f literals=%.0f sequences=%.0f\n", h[0],
                              (double)h[1] / h[0], (double)h[2] / h[0], (double)h[3] / h[0], (double)h[4] / h[0]);
        });
    return a;
}
static GatherArgs rounds_gather_args(znippy_ctx *ctx, const znippy_rounds *r, const EncPlan &p, const EncRun &run) {
    GatherArgs g{};
    g.items = r->items; g.n_pieces = r->n_items; g.piece_len = r->piece_len; g.piece_start = r->piece_start;
    g.local_excl = r->local_excl; g.block_tot = r->block_tot; g.prov = ctx->enc_prov;
    g.src = (const uint8_t *)run.d_src; g.src_off = r->src_off;
    g.blob_out = (uint8_t *)run.d_blob_out; g.blob_cap = run.blob_cap;
    g.blob_offset = run.res.blob_offset(); g.blob_size = run.res.blob_size(); g.total = run.res.total(); g.overflow = run.res.overflow();
    g.stored = p.store_decide ? r->stored : nullptr;
    g.skip_stored_copy = p.fuse_store ? 1 : 0;
    g.pad = run.pad;
    g.small_pieces = p.small_pieces ? 1 : 0;
    return g;
}

static int enc_clear(znippy_ctx *ctx, znippy_rounds *r, const EncPlan &, const EncRun &run) {
    hipStream_t s = ctx->stream;
    if (r->run_seq >= 2) HIPCHK(ctx, hipStreamWaitEvent(s, r->ev_res[run.slot], 0));  // the slab's previous results have left
    HIPCHK(ctx, hipMemsetAsync(run.res.base, 0, ResSlab::clear_bytes(r->n), s));  // total, overflow, blob_offset, blob_size
    HIPCHK(ctx, hipMemsetAsync(ctx->cursor, 0, 64, s));  // work cursors + (last word) the count of blocks handed to the wide variant
    // The fork comes AFTER the clears.  The hash kernel on the auxiliary stream starts at the fork and fills the chip; a
    // clear issued behind it is one tiny fill kernel that then waits ~100 us for its turn (kernel trace of the C2 write
    // step: two of them, 88 + 125 us, between the previous run's gather and this run's encoder).
    HIPCHK(ctx, hipEventRecord(ctx->ev_fork, s));
    return ZNIPPY_OK;
}

static int enc_far_index(znippy_ctx *ctx, znippy_rounds *r, const EncPlan &p, const EncRun &run) {
    if (!p.far) return ZNIPPY_OK;
    ktime_begin(ctx, "ldm_index");
    HIPCHK(ctx, hipMemsetAsync(ctx->ldm, 0xFF, 4 * r->ldm_entries, ctx->stream));
    launch_ldm_index(r->d_ldm, (uint32_t)r->h_ldm.size(), r->ldm_chunks, (const uint8_t *)run.d_src, r->src_off, r->len, ctx->ldm, ctx->stream);
    ktime_end(ctx);
    return ZNIPPY_OK;
}

// the wide share first (its blocks are the long ones), the small share, then whatever the small variant handed over
static void enc_blocks(znippy_ctx *ctx, znippy_rounds *r, const EncPlan &p, const EncRun &run) {
    hipStream_t s = ctx->stream;
    EncodeArgs a = rounds_encode_args(ctx, r, p, run);
    ktime_begin(ctx, p.fuse_hash ? "zstd_encode_hash" : "zstd_encode");
    if (p.wide.on) {
        a.n_items = p.wide.n_items; a.order = p.wide.use_order ? r->order_wide : nullptr;
        a.cursor = ctx->cursor + 8; a.batch = p.wide.batch;
        launch_encode(a, p.wide.grid, false, p.high, s);
    }
    if (p.small.on) {
        a.n_items = p.small.n_items; a.order = p.small.use_order ? r->order_small : nullptr;
        a.cursor = ctx->cursor; a.batch = p.small.batch;
        a.retry_list = r->retry_list; a.retry_count = ctx->cursor + 15;
        if (p.fuse_hash) { a.fuse_tiles = r->fuse_tiles; a.h = rounds_hash_args(r, run.res, run.d_src); }
        launch_encode(a, p.small.grid, true, p.high, s);
        a.fuse_tiles = 0;
    }
    if (p.retry.on) {
        a.order = r->retry_list; a.n_items = p.retry.n_items; a.n_items_dev = ctx->cursor + 15;
        a.retry_list = nullptr; a.retry_count = nullptr;
        a.cursor = ctx->cursor + 12; a.batch = p.retry.batch;
        launch_encode(a, p.retry.grid, false, p.high, s);
    }
    ktime_end(ctx);
}

static int enc_hash_beside(znippy_ctx *ctx, znippy_rounds *r, const EncPlan &p, const EncRun &run) {
    if (!p.fork_aux) return ZNIPPY_OK;
    HIPCHK(ctx, hipStreamWaitEvent(ctx->aux, ctx->ev_fork, 0));
    const int rc = p.hash_beside ? hash_rounds_async(ctx, r, run.res, run.d_src, ctx->aux, nullptr, 0, 1, run.tree_out) : ZNIPPY_OK;
    if (rc) return rc;
    HIPCHK(ctx, hipEventRecord(ctx->ev_join, ctx->aux));
    return ZNIPPY_OK;
}

// where every piece goes: the opt-in passes that change lengths, then the scan
static void enc_layout(znippy_ctx *ctx, znippy_rounds *r, const EncPlan &p, const EncRun &run) {
    hipStream_t s = ctx->stream;
    if (p.store_decide)
        timed(ctx, "store_decide", s, [&] { launch_store_decide(r->first_item, r->items, r->len, r->skip, r->n, r->piece_len, r->stored, s); });
    if (p.pad)
        timed(ctx, "round_pad", s, [&] {
            launch_round_pad(r->first_item, r->items, r->len, r->skip, p.store_decide ? r->stored : nullptr, r->n, r->piece_len, run.align, r->piece_pad, s);
        });
    timed(ctx, "piece_scan", s, [&] { launch_piece_scan(r->piece_len, run.pad, r->n_items, r->local_excl, r->block_tot, s); });
}

static void enc_gather(znippy_ctx *ctx, znippy_rounds *r, const EncPlan &p, const EncRun &run) {
    const GatherArgs g = rounds_gather_args(ctx, r, p, run);
    timed(ctx, "gather", ctx->stream, [&] { launch_gather(g, ctx->stream); });
}

// the fused-store hash behind the gather, or the join of the hash beside
static int enc_hash_store(znippy_ctx *ctx, znippy_rounds *r, const EncPlan &p, const EncRun &run) {
    if (p.fuse_store) return hash_rounds_async(ctx, r, run.res, run.d_src, nullptr, run.d_blob_out, run.blob_cap, run.align, run.tree_out);
    if (p.fork_aux) HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));  // digests are complete once the main stream drains
    return ZNIPPY_OK;
}

// the results leave on the copy stream (into the slot's pinned mirror) while the main stream is free for the next run
static int enc_results_out(znippy_ctx *ctx, znippy_rounds *r, const EncPlan &, const EncRun &run) {
    HIPCHK(ctx, hipEventRecord(r->ev_enc[run.slot], ctx->stream));
    HIPCHK(ctx, hipStreamWaitEvent(ctx->copy, r->ev_enc[run.slot], 0));
    const uint32_t n16 = (uint32_t)((r->res_bytes + 15) / 16);  // both buffers are allocated in whole 16-byte units and more
    // few workgroups: the copy only has to be done before the next run but one needs the slab, and it shares the chip with
    // the next run's kernels (4-16 workgroups: 0.84 ms per C2 write step, 64: 0.88, 1,024: 0.90)
    hipLaunchKernelGGL(k_results_out, dim3(std::min<uint32_t>((n16 + 255) / 256, 8)), dim3(256), 0, ctx->copy,
                       reinterpret_cast<uint4 *>(r->h_res_m[run.slot]), reinterpret_cast<const uint4 *>(run.res.base), n16);
    if (run.tree_out) {  // the tree leaves with the results, in front of ev_res: the slab-reuse wait covers its buffer too
        const uint32_t t16 = 2 * r->n_tree_entries;
        hipLaunchKernelGGL(k_results_out, dim3(std::min<uint32_t>((t16 + 255) / 256, 8)), dim3(256), 0, ctx->copy,
                           reinterpret_cast<uint4 *>(r->h_tree_m[run.slot]), reinterpret_cast<const uint4 *>(run.tree_out), t16);
    }
    HIPCHK(ctx, hipEventRecord(r->ev_res[run.slot], ctx->copy));
    return ZNIPPY_OK;
}

// Queues one run of the table into slot `slot`.  Every allocation the run needs is made before its first stream operation
// (*queued): an error return after that point is a HIP runtime error, which the caller turns into a table whose latest run is
// still the one before (rounds_abandon).  Only a run queued to its end enters the table's books.
static int rounds_launch(znippy_ctx *ctx, znippy_rounds *r, const void *d_src, void *d_blob_out, uint64_t blob_cap, unsigned slot, bool *queued) {
    ctx->n_ktimes = 0;
    if (!r->n) return ZNIPPY_OK;
    int rc = ensure_encoder(ctx);
    if (rc) return rc;
    EncEnv env{ctx->level, ctx->window_log, ctx->encode_grid, ctx->encode_grid_small, (bool)ctx->sw.nohash, (bool)ctx->sw.no_fuse_hash, (bool)ctx->sw.no_fused_store, false};
    env.ldm_ok = enc_window_log(env) && ensure_ldm(ctx, r);
    if (r->prov_bytes + 64 > ctx->enc_prov_cap) {
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->enc_prov) (void)hipFree(ctx->enc_prov);
        ctx->enc_prov = nullptr; ctx->enc_prov_cap = 0;
        HIPCHK(ctx, hipMalloc(&ctx->enc_prov, r->prov_bytes + 64));
        ctx->enc_prov_cap = r->prov_bytes + 64;
        if (ctx->sw.poison) HIPCHK(ctx, poison_dev(ctx, ctx->enc_prov, ctx->enc_prov_cap));
    }
    const EncPlan p = enc_plan(rounds_shape(r), env);
    // the alignment and the tree switch are this run's values: a later znippy_rounds_set_blob_align / _emit_block_tree does not reach it
    const EncRun run{d_src, d_blob_out, blob_cap, slot, r->dev(slot), p.tree_out ? r->tree_m[slot] : nullptr, r->blob_align, p.pad ? r->piece_pad : nullptr};
    *queued = true;
    if ((rc = enc_clear(ctx, r, p, run)) || (rc = enc_far_index(ctx, r, p, run))) return rc;
    enc_blocks(ctx, r, p, run);
    if ((rc = enc_hash_beside(ctx, r, p, run))) return rc;
    enc_layout(ctx, r, p, run);
    enc_gather(ctx, r, p, run);
    if ((rc = enc_hash_store(ctx, r, p, run)) || (rc = enc_results_out(ctx, r, p, run))) return rc;
    HIPCHK(ctx, hipGetLastError());
    r->tree_run[slot] = p.emit_tree;
    r->slot = slot;
    r->run_seq++;
    return ZNIPPY_OK;
}

// A run that failed after its first stream operation: the auxiliary stream is joined back into the main one, the copy stream
// gets behind the run's end if that was recorded (a wait for an event never recorded is none), everything is waited for and
// the sticky error cleared.  The table's books are as before the call; the failed run's slot — the run before last — may hold
// a part of it.
static void rounds_abandon(znippy_ctx *ctx, znippy_rounds *r, unsigned slot) {
    if (hipEventRecord(ctx->ev_join, ctx->aux) == hipSuccess) (void)hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0);
    (void)hipStreamWaitEvent(ctx->copy, r->ev_enc[slot], 0);
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipStreamSynchronize(ctx->copy);
    (void)hipGetLastError();
}
static int rounds_queue(znippy_ctx *ctx, znippy_rounds *r, const void *d_src, void *d_blob_out, uint64_t blob_cap) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    { const int prc = poison_enter(ctx); if (prc) return prc; }
    const unsigned slot = (unsigned)(r->run_seq & 1);
    bool queued = false;
    const int rc = rounds_launch(ctx, r, d_src, d_blob_out, blob_cap, slot, &queued);
    if (rc && queued) rounds_abandon(ctx, r, slot);
    return rc;
}

extern "C" int znippy_encode_hash_rounds_async(znippy_ctx *ctx, znippy_rounds *r, const void *d_src, void *d_blob_out,
                                               uint64_t blob_cap) {
    if (!ctx_enter(ctx)) return ZNIPPY_E_INVAL;
    if (!ctx || !r || r->ctx != ctx || (r->n && (!d_src || !d_blob_out))) return ZNIPPY_E_INVAL;
    return rounds_queue(ctx, r, d_src, d_blob_out, blob_cap);
}

// The header of a finished run's mirror: the blob bytes, or ZNIPPY_E_DST_SMALL when the run ran out of blob_cap.
static int res_header(const ResSlab &h, uint64_t *total) {
    uint32_t ovf;
    memcpy(total, h.total(), 8);
    memcpy(&ovf, h.overflow(), 4);
    return ovf ? ZNIPPY_E_DST_SMALL : ZNIPPY_OK;
}
static void res_view(const ResSlab &h, const uint64_t **blob_offset, const uint64_t **blob_size, const uint8_t **checksum) {
    if (blob_offset) *blob_offset = h.blob_offset();
    if (blob_size) *blob_size = h.blob_size();
    if (checksum) *checksum = reinterpret_cast<const uint8_t *>(h.digests());
}

// Results of the run `lag` runs before the latest one (0 or 1) as pointers into that run's pinned mirror; waits for
// that run's copy only.  Valid until two more encode calls have been queued on the table.
extern "C" int znippy_rounds_results_lagged(znippy_ctx *ctx, znippy_rounds *r, unsigned lag, const uint64_t **blob_offset,
                                            const uint64_t **blob_size, const uint8_t **checksum, uint64_t *blob_bytes) {
    if (!ctx_enter(ctx)) return ZNIPPY_E_INVAL;
    if (!ctx || !r || r->ctx != ctx || lag > 1 || r->run_seq <= lag) return ZNIPPY_E_INVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const unsigned slot = (unsigned)((r->run_seq - 1 - lag) & 1);
    HIPCHK(ctx, hipEventSynchronize(r->ev_res[slot]));
    uint64_t total;
    const int rc = res_header(r->host(slot), &total);
    if (rc) return rc;
    res_view(r->host(slot), blob_offset, blob_size, checksum);
    if (blob_bytes) *blob_bytes = total;
    return ZNIPPY_OK;
}

extern "C" int znippy_rounds_results(znippy_ctx *ctx, znippy_rounds *r, uint64_t *blob_offset, uint64_t *blob_size,
                                     uint8_t *checksum, uint8_t *compressed, uint64_t *blob_bytes) {
    if (!ctx_enter(ctx)) return ZNIPPY_E_INVAL;
    if (!ctx || !r || r->ctx != ctx) return ZNIPPY_E_INVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (blob_bytes) *blob_bytes = 0;
    if (!r->n) return ZNIPPY_OK;
    if (!r->run_seq) return ZNIPPY_E_INVAL;  // nothing has been encoded on this table yet
    HIPCHK(ctx, hipEventSynchronize(r->ev_res[r->slot]));  // the latest run's results have arrived
    if (r->store_incompressible) {
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        HIPCHK(ctx, hipMemcpy(r->h_stored, r->stored, r->n, hipMemcpyDeviceToHost));
    }
    const ResSlab h = r->host(r->slot);
    uint64_t total;
    const int rc = res_header(h, &total);
    if (rc) return rc;
    const size_t n = r->n;
    if (blob_offset) memcpy(blob_offset, h.blob_offset(), 8 * n);
    if (blob_size) memcpy(blob_size, h.blob_size(), 8 * n);
    if (checksum) memcpy(checksum, h.digests(), 32 * n);
    if (compressed)
        for (uint32_t i = 0; i < r->n; i++)
            compressed[i] = ((!r->h_skip.empty() && r->h_skip[i]) || (r->store_incompressible && r->h_stored[i])) ? 0 : 1;
    if (blob_bytes) *blob_bytes = total;
    return ZNIPPY_OK;
}

// Zero-copy variant: pointers into the table's pinned result mirror, valid until the next encode call
// on this table (compressed[] = !skip is known to the caller already).
extern "C" int znippy_rounds_results_view(znippy_ctx *ctx, znippy_rounds *r, const uint64_t **blob_offset,
                                          const uint64_t **blob_size, const uint8_t **checksum, uint64_t *blob_bytes) {
    if (!ctx_enter(ctx)) return ZNIPPY_E_INVAL;
    int rc = znippy_rounds_results(ctx, r, nullptr, nullptr, nullptr, nullptr, blob_bytes);
    if (rc) return rc;
    res_view(r->host(r->slot), blob_offset, blob_size, checksum);
    return ZNIPPY_OK;
}

extern "C" int znippy_encode_hash_rounds(znippy_ctx *ctx, znippy_rounds *rounds, const void *d_src, void *d_blob_out,
                                         uint64_t blob_cap, uint64_t *blob_offset, uint64_t *blob_size,
                                         uint8_t *checksum, uint8_t *compressed, uint64_t *blob_bytes) {
    if (!ctx_enter(ctx)) return ZNIPPY_E_INVAL;
    int rc = znippy_encode_hash_rounds_async(ctx, rounds, d_src, d_blob_out, blob_cap);
    if (rc) return rc;
    return znippy_rounds_results(ctx, rounds, blob_offset, blob_size, checksum, compressed, blob_bytes);
}

extern "C" int znippy_compress(znippy_ctx *ctx, const void *src, size_t n, void *dst, size_t cap, size_t *written) {
    if (!ctx_enter(ctx)) return ZNIPPY_E_INVAL;
    if (!ctx || !written || !dst || (n && !src)) return ZNIPPY_E_INVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t bound = znippy_compress_bound(n);
    int rc = shim_reserve(ctx, n, bound);
    if (rc) return rc;
    if (n) HIPCHK(ctx, hipMemcpyAsync(ctx->shim_in, src, n, hipMemcpyHostToDevice, ctx->stream));
    uint64_t off = 0, len = n, bsz = 0, total = 0;
    znippy_rounds *r = nullptr;
    rc = znippy_rounds_create(ctx, &off, &len, nullptr, 1, &r);
    if (rc) return rc;
    rc = znippy_encode_hash_rounds(ctx, r, ctx->shim_in, ctx->shim_out, ctx->shim_out_cap, nullptr, &bsz, nullptr, nullptr,
                                   &total);
    znippy_rounds_destroy(r);
    if (rc) return rc;
    if (total > cap) return ZNIPPY_E_DST_SMALL;
    HIPCHK(ctx, hipMemcpy(dst, ctx->shim_out, total, hipMemcpyDeviceToHost));
    *written = total;
    return ZNIPPY_OK;
}

extern "C" size_t znippy_compress_bound(size_t n) {
    // every 128 KiB block can fall back to a raw block (3-byte header) + frame header (<= 13) + the empty closing block
    // the higher effort tier puts behind frames of several blocks
    return n + 3 * (n / BLOCK_BYTES + 1) + 19;
}

extern "C" int znippy_rounds_set_blob_align(znippy_rounds *r, uint32_t align) {
    if (!r || !r->ctx || !ctx_enter(r->ctx) || align < 1 || align > 4096 || (align & (align - 1))) return ZNIPPY_E_INVAL;
    znippy_ctx *const ctx = r->ctx;
    if (align > 1 && !r->piece_pad) {  // cleared once, on the stream the runs are queued on
        HIPCHK(ctx, hipSetDevice(ctx->device));
        const size_t bytes = 4 * std::max<size_t>(r->n_items, 4);
        uint32_t *p = nullptr;
        if (tmalloc(ctx, &p, bytes) != hipSuccess) return ZNIPPY_E_NOMEM;
        if (hipMemsetAsync(p, 0, bytes, ctx->stream) != hipSuccess) { (void)hipGetLastError(); tfree(ctx, p); return ZNIPPY_E_HIP; }
        r->piece_pad = p;
    }
    r->blob_align = align;
    return ZNIPPY_OK;
}

extern "C" uint32_t znippy_rounds_blob_align(const znippy_rounds *r) { return r ? r->blob_align : 1; }

// ---- block tree of a rounds table -------------------------------------------------------------------
// The layout needs the lengths on the host; the table keeps them on the device only, so the first call that asks fetches them.
static int rounds_tree_layout(znippy_ctx *ctx, znippy_rounds *r) {
    if (!r->tree_first.empty()) return ZNIPPY_OK;
    std::vector<uint64_t> len(r->n), first((size_t)r->n + 1, 0);
    if (r->n) HIPCHK(ctx, hipMemcpy(len.data(), r->len, 8 * (size_t)r->n, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < r->n; i++) first[i + 1] = first[i] + tree_entries_of(len[i]);
    r->tree_first.swap(first);
    return ZNIPPY_OK;
}

static int rounds_block_tree_layout(znippy_ctx *ctx, znippy_rounds *r, uint64_t *n_entries, uint64_t *round_first) {
    if (!ctx_enter(ctx)) return ZNIPPY_E_INVAL;
    if (!ctx || !r || r->ctx != ctx || !n_entries) return ZNIPPY_E_INVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int rc = rounds_tree_layout(ctx, r);
    if (rc) return rc;
    *n_entries = r->tree_first[r->n];
    if (round_first) memcpy(round_first, r->tree_first.data(), 8 * ((size_t)r->n + 1));
    return ZNIPPY_OK;
}

// Everything the feature needs, once per table: the list of units with entries and, per slot of the two-run ring, a device tree
// buffer and its pinned mirror.  A failure leaves the table as it was (emission off, nothing kept).
static int rounds_emit_block_tree(znippy_rounds *r, int on) {
    if (!r || !r->ctx || !ctx_enter(r->ctx)) return ZNIPPY_E_INVAL;
    znippy_ctx *const ctx = r->ctx;
    if (!on || r->tree_ready) { r->emit_tree = on != 0; return ZNIPPY_OK; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = rounds_tree_layout(ctx, r);
    if (rc) return rc;
    const uint64_t n_entries = r->tree_first[r->n];
    if (n_entries) {
        if (n_entries > 0x7FFFFFF0ull) return ZNIPPY_E_NOMEM;
        std::vector<BigUnit> big(r->plan.n_big);
        HIPCHK(ctx, hipMemcpy(big.data(), r->plan.big, sizeof(BigUnit) * big.size(), hipMemcpyDeviceToHost));
        std::vector<TreeUnit> units;
        for (const BigUnit &b : big) {  // (in round order, as the tree is)
            const uint64_t first = r->tree_first[b.unit], cnt = r->tree_first[(size_t)b.unit + 1] - first;
            if (!cnt) continue;  // one block (n_cvs <= 2), or 4 GiB and more
            if (cnt != ((uint64_t)b.n_cvs + 1) / 2) return ZNIPPY_E_INVAL;  // (the plan and the layout are cut from the same lengths)
            units.push_back(TreeUnit{(uint32_t)first, b.cv_base, b.n_cvs, 0});
        }
        units.push_back(TreeUnit{(uint32_t)n_entries, 0, 0, 0});
        struct Guard {  // (nothing below is kept unless all of it succeeds)
            znippy_ctx *ctx; TreeUnit *units = nullptr; uint32_t *tree[2] = {nullptr, nullptr}; void *h[2] = {nullptr, nullptr}; size_t cap[2] = {0, 0};
            ~Guard() { tfree(ctx, units); for (int k = 0; k < 2; k++) { tfree(ctx, tree[k]); pinned_give(ctx, h[k], cap[k]); } }
        } g{ctx};
        if (tmalloc(ctx, &g.units, sizeof(TreeUnit) * units.size()) != hipSuccess) return ZNIPPY_E_NOMEM;
        for (int k = 0; k < 2; k++)
            if (tmalloc(ctx, &g.tree[k], 32 * (size_t)n_entries) != hipSuccess || !(g.h[k] = pinned_take(ctx, 32 * (size_t)n_entries, &g.cap[k]))) return ZNIPPY_E_NOMEM;
        HIPCHK(ctx, hipMemcpy(g.units, units.data(), sizeof(TreeUnit) * units.size(), hipMemcpyHostToDevice));
        r->tree_units = g.units; g.units = nullptr;
        r->n_tree_units = (uint32_t)units.size() - 1;
        for (int k = 0; k < 2; k++) {
            r->tree_m[k] = g.tree[k]; g.tree[k] = nullptr;
            r->h_tree_m[k] = (uint8_t *)g.h[k]; g.h[k] = nullptr;
            r->h_tree_cap_m[k] = g.cap[k];
        }
        r->n_tree_entries = (uint32_t)n_entries;
    }
    r->tree_ready = true;
    r->emit_tree = true;
    return ZNIPPY_OK;
}

static int rounds_block_tree(znippy_ctx *ctx, znippy_rounds *r, unsigned lag, uint8_t *tree) {
    if (!ctx_enter(ctx)) return ZNIPPY_E_INVAL;
    if (!ctx || !r || r->ctx != ctx || lag > 1 || r->run_seq <= lag) return ZNIPPY_E_INVAL;
    const unsigned slot = (unsigned)((r->run_seq - 1 - lag) & 1);
    if (!r->tree_run[slot]) return ZNIPPY_E_INVAL;  // that run was queued with emission off
    if (!r->n_tree_entries) return ZNIPPY_OK;
    if (!tree) return ZNIPPY_E_INVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipEventSynchronize(r->ev_res[slot]));  // that run's result copy, which the tree travels with
    memcpy(tree, r->h_tree_m[slot], 32 * (size_t)r->n_tree_entries);
    return ZNIPPY_OK;
}

extern "C" int znippy_rounds_emit_block_tree(znippy_rounds *r, int on) { ZN_NO_THROW(rounds_emit_block_tree(r, on)) }
extern "C" int znippy_rounds_block_tree_layout(znippy_ctx *ctx, znippy_rounds *r, uint64_t *n_entries, uint64_t *round_first) {
    ZN_NO_THROW(rounds_block_tree_layout(ctx, r, n_entries, round_first))
}
extern "C" int znippy_rounds_block_tree(znippy_ctx *ctx, znippy_rounds *r, unsigned lag, uint8_t *tree) { ZN_NO_THROW(rounds_block_tree(ctx, r, lag, tree)) }

extern "C" int znippy_rounds_set_store_incompressible(znippy_rounds *r, int on) {
    if (!r) return ZNIPPY_E_INVAL;
    r->store_incompressible = on != 0;
    return ZNIPPY_OK;
}

// ---- the DEFLATE batch calls: not runs, no table is involved -------------------------------------------
// What each call works out on the host — which items pass, where they go, the lists the kernels read, what the kernels' answers mean
// — is host/deflate_batch.{h,cc}, plain C++ that a stand-alone program tests.  Here: the argument checks, the allocations, the
// copies and the launches, in stages over that plan.
static_assert(DB_OK == ZNIPPY_OK && DB_E_INVAL == ZNIPPY_E_INVAL && DB_E_NOMEM == ZNIPPY_E_NOMEM && DB_E_DST_SMALL == ZNIPPY_E_DST_SMALL &&
              DB_E_CORRUPT == ZNIPPY_E_CORRUPT && DB_E_UNSUPPORTED == ZNIPPY_E_UNSUPPORTED && DB_E_CHECKSUM == ZNIPPY_E_CHECKSUM,
              "host/deflate_batch.h gives out the codes of znippy_hip.h");
static_assert(gzp::OK == ZNIPPY_OK && gzp::E_DST_SMALL == ZNIPPY_E_DST_SMALL && gzp::E_CORRUPT == ZNIPPY_E_CORRUPT &&
              gzp::E_UNSUPPORTED == ZNIPPY_E_UNSUPPORTED && gzp::E_CHECKSUM == ZNIPPY_E_CHECKSUM, "host/gz_plan.h gives out the codes of znippy_hip.h");

// ---- raw DEFLATE of ZIP entries (znippy_inflate_batch) ---------------------------------------------
// The items that pass inflate_admit are uploaded as one list, decoded by one launch (wave = stream) and checksummed by a second one;
// status and CRC come back in one copy each.
static int inflate_batch(znippy_ctx *ctx, const void *d_src, uint64_t src_cap, const uint64_t *src_off, const uint64_t *src_len,
                         const uint8_t *method, void *d_out, uint64_t out_cap, const uint64_t *out_off, const uint64_t *out_len,
                         const uint32_t *crc32, uint64_t n, int32_t *status, uint32_t *crc_out) {
    if (!ctx_enter(ctx)) return ZNIPPY_E_INVAL;
    if (!ctx || n >= 0xFFFFFFF0ull) return ZNIPPY_E_INVAL;
    if (!n) return ZNIPPY_OK;
    if (!src_off || !src_len || !out_len || !d_src || !d_out) return ZNIPPY_E_INVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    ctx->n_ktimes = 0;
    { const int prc = poison_enter(ctx); if (prc) return prc; }

    InflateBatch b;
    inflate_admit(InflateCall{(const uint8_t *)d_src, src_cap, src_off, src_len, method, (uint8_t *)d_out, out_cap, out_off, out_len, crc32, n}, b);
    const uint32_t n_items = (uint32_t)b.items.size();
    if (n_items) {  // every allocation, then the stream
        struct Guard {
            znippy_ctx *ctx;
            InflateItem *items = nullptr; int32_t *st = nullptr; uint32_t *crc = nullptr;
            ~Guard() { tfree(ctx, items); tfree(ctx, st); tfree(ctx, crc); }
        } g{ctx};
        HIPCHK(ctx, tmalloc(ctx, &g.items, sizeof(InflateItem) * n_items));
        HIPCHK(ctx, tmalloc(ctx, &g.st, sizeof(int32_t) * n_items));
        HIPCHK(ctx, tmalloc(ctx, &g.crc, sizeof(uint32_t) * n_items));
        HIPCHK(ctx, hipMemcpyAsync(g.items, b.items.data(), sizeof(InflateItem) * n_items, hipMemcpyHostToDevice, s));
        HIPCHK(ctx, hipMemsetAsync(g.crc, 0, sizeof(uint32_t) * n_items, s));
        timed(ctx, "inflate", s, [&] { launch_inflate(g.items, n_items, g.st, s); });
        timed(ctx, "inflate_crc", s, [&] { launch_inflate_crc(g.items, n_items, g.st, g.crc, s); });
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(b.h_st.data(), g.st, sizeof(int32_t) * n_items, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipMemcpyAsync(b.h_crc.data(), g.crc, sizeof(uint32_t) * n_items, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
    }
    inflate_scatter(b, n, status, crc_out);
    return ZNIPPY_OK;
}

extern "C" int znippy_inflate_batch(znippy_ctx *ctx, const void *d_src, uint64_t src_cap, const uint64_t *src_off, const uint64_t *src_len,
                                    const uint8_t *method, void *d_out, uint64_t out_cap, const uint64_t *out_off, const uint64_t *out_len,
                                    const uint32_t *crc32, uint64_t n, int32_t *status, uint32_t *crc_out) {
    ZN_NO_THROW(inflate_batch(ctx, d_src, src_cap, src_off, src_len, method, d_out, out_cap, out_off, out_len, crc32, n, status, crc_out))
}

// ---- one tar member out of gzip-compressed tars (znippy_targz_find_batch) ----------------------------
// The items that pass targz_admit get a slice of the context's range scratch (sized before anything is queued) and are walked by one
// launch (wave = stream, targz.hip); status, place and length come back in one copy; the members that targz_pack finds in place and
// fitting are packed into d_out by the range reads' gather.
static int targz_find_batch(znippy_ctx *ctx, const void *d_src, uint64_t src_cap, const uint64_t *src_off, const uint64_t *src_len, const uint8_t *whole,
                            uint64_t n, const char *name_prefix, uint64_t prefix_len, const char *name_suffix, uint64_t suffix_len, uint64_t scan_cap,
                            void *d_out, uint64_t out_cap, uint64_t *out_off, uint64_t *out_len, int32_t *status, uint64_t *scanned) {
    if (!ctx_enter(ctx)) return ZNIPPY_E_INVAL;
    if (!ctx || n >= 0xFFFFFFF0ull) return ZNIPPY_E_INVAL;
    if (!n) return ZNIPPY_OK;
    if (!src_off || !src_len || !out_off || !out_len || !d_src || (out_cap && !d_out) || (prefix_len && !name_prefix) || (suffix_len && !name_suffix) ||
        prefix_len >= (1u << 16) || suffix_len >= (1u << 16) || scan_cap < 512)
        return ZNIPPY_E_INVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    ctx->n_ktimes = 0;
    { const int prc = poison_enter(ctx); if (prc) return prc; }

    const TargzCall call{(const uint8_t *)d_src, src_cap, src_off, src_len, whole, n, scan_cap, (uint8_t *)d_out, out_cap, out_off, out_len, scanned};
    TargzBatch b;
    int rc;
    if ((rc = targz_admit(call, b))) return rc;
    const uint32_t n_items = (uint32_t)b.items.size();
    if (n_items) {  // every allocation, then the stream
        if ((rc = ensure_range_scratch(ctx, 0, b.need))) return rc;
        targz_bind(b, ctx->rr_pool[0]);
        struct Guard {
            znippy_ctx *ctx;
            TargzItem *items = nullptr; TargzResult *res = nullptr; uint8_t *filter = nullptr; RangePiece *pieces = nullptr;
            ~Guard() { tfree(ctx, items); tfree(ctx, res); tfree(ctx, filter); tfree(ctx, pieces); }
        } g{ctx};
        std::vector<uint8_t> filter(prefix_len + suffix_len + 16, 0);
        if (prefix_len) memcpy(filter.data(), name_prefix, prefix_len);
        if (suffix_len) memcpy(filter.data() + prefix_len, name_suffix, suffix_len);
        size_t max_pieces;  // the gather's list is cut once the results are known
        if ((rc = targz_piece_bound(out_cap, n_items, &max_pieces))) return rc;
        HIPCHK(ctx, tmalloc(ctx, &g.items, sizeof(TargzItem) * n_items));
        HIPCHK(ctx, tmalloc(ctx, &g.res, sizeof(TargzResult) * n_items));
        HIPCHK(ctx, tmalloc(ctx, &g.filter, filter.size()));
        HIPCHK(ctx, tmalloc(ctx, &g.pieces, sizeof(RangePiece) * max_pieces));
        HIPCHK(ctx, hipMemcpyAsync(g.items, b.items.data(), sizeof(TargzItem) * n_items, hipMemcpyHostToDevice, s));
        HIPCHK(ctx, hipMemcpyAsync(g.filter, filter.data(), filter.size(), hipMemcpyHostToDevice, s));
        timed(ctx, "targz_find", s, [&] { launch_targz_find(g.items, n_items, g.filter, (uint32_t)prefix_len, (uint32_t)suffix_len, g.res, s); });
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(b.res.data(), g.res, sizeof(TargzResult) * n_items, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
        targz_pack(call, b);
        if (!b.pieces.empty()) {
            if (b.pieces.size() > max_pieces) return ZNIPPY_E_NOMEM;  // (cannot happen: the bound counts them)
            HIPCHK(ctx, hipMemcpyAsync(g.pieces, b.pieces.data(), sizeof(RangePiece) * b.pieces.size(), hipMemcpyHostToDevice, s));
            timed(ctx, "targz_gather", s, [&] { launch_range_gather(g.pieces, (uint32_t)b.pieces.size(), s); });
            HIPCHK(ctx, hipGetLastError());
            HIPCHK(ctx, hipStreamSynchronize(s));
        }
    }
    if (status) memcpy(status, b.st.data(), sizeof(int32_t) * n);
    return ZNIPPY_OK;
}

extern "C" int znippy_targz_find_batch(znippy_ctx *ctx, const void *d_src, uint64_t src_cap, const uint64_t *src_off, const uint64_t *src_len,
                                       const uint8_t *whole, uint64_t n, const char *name_prefix, uint64_t prefix_len, const char *name_suffix,
                                       uint64_t suffix_len, uint64_t scan_cap, void *d_out, uint64_t out_cap, uint64_t *out_off, uint64_t *out_len,
                                       int32_t *status, uint64_t *scanned) {
    ZN_NO_THROW(targz_find_batch(ctx, d_src, src_cap, src_off, src_len, whole, n, name_prefix, prefix_len, name_suffix, suffix_len, scan_cap, d_out, out_cap,
                                 out_off, out_len, status, scanned))
}

// ---- whole gzip files (znippy_gunzip_batch) ----------------------------------------------------------
// The items that pass gz_admit are scanned for candidate starts; gz_candidates keeps candidates and says which items are probed and
// which take the single pass (those without a kept candidate behind byte 0, and those whose candidates did not fit their slice of the
// list); the probe leaves a record per kept candidate; gz_decode_plan turns records into runs and members, and the decode and CRC
// launches follow; gz_verdict reads their answers.  One device allocation (gz_layout), sized from the source lengths before anything
// is queued, holds every list.
struct GzDev {  // the allocation, and where its lists are
    uint8_t *p;
    GzLayout at;
    hipStream_t s;
    template <typename T>
    T *list(size_t off) const { return (T *)(p + off); }
    const GzItem *items() const { return list<GzItem>(at.items); }
};

// items and chunks up; the scan; the counts back, then the raw list as far as gz_raw_end says
static int gz_scan_stage(znippy_ctx *ctx, GzBatch &b, const GzDev &d) {
    const uint32_t n_items = (uint32_t)b.items.size();
    hipStream_t s = d.s;
    HIPCHK(ctx, hipMemcpyAsync(d.p + d.at.items, b.items.data(), sizeof(GzItem) * n_items, hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(d.p + d.at.chunks, b.chunks.data(), sizeof(GzScanChunk) * b.chunks.size(), hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipMemsetAsync(d.p + d.at.count, 0, sizeof(uint32_t) * n_items, s));
    timed(ctx, "gunzip_scan", s, [&] {
        launch_gunzip_scan(d.items(), d.list<const GzScanChunk>(d.at.chunks), (uint32_t)b.chunks.size(), d.list<uint32_t>(d.at.count), d.list<uint64_t>(d.at.raw), s);
    });
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(b.count.data(), d.p + d.at.count, sizeof(uint32_t) * n_items, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    if (const uint64_t raw_end = gz_raw_end(b)) {
        b.raw.resize(raw_end);
        HIPCHK(ctx, hipMemcpyAsync(b.raw.data(), d.p + d.at.raw, sizeof(uint64_t) * raw_end, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
    }
    return ZNIPPY_OK;
}

// the probe over the kept candidates, the single pass over the other items; records and results back
static int gz_probe_stage(znippy_ctx *ctx, GzBatch &b, const GzDev &d) {
    const uint32_t n_cands = (uint32_t)b.cands.size(), n_single = (uint32_t)b.single.size();
    hipStream_t s = d.s;
    if (n_cands) {
        HIPCHK(ctx, hipMemcpyAsync(d.p + d.at.cands, b.cands.data(), sizeof(GzCand) * n_cands, hipMemcpyHostToDevice, s));
        if (!b.stops.empty()) HIPCHK(ctx, hipMemcpyAsync(d.p + d.at.stops, b.stops.data(), sizeof(uint32_t) * b.stops.size(), hipMemcpyHostToDevice, s));
        timed(ctx, "gunzip_probe", s, [&] {
            launch_gunzip_probe(d.items(), d.list<const GzCand>(d.at.cands), n_cands, d.list<const uint32_t>(d.at.stops), d.list<GzProbe>(d.at.recs), s);
        });
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(b.recs.data(), d.p + d.at.recs, sizeof(GzProbe) * n_cands, hipMemcpyDeviceToHost, s));
    }
    if (n_single) {
        HIPCHK(ctx, hipMemcpyAsync(d.p + d.at.single_list, b.single.data(), sizeof(uint32_t) * n_single, hipMemcpyHostToDevice, s));
        timed(ctx, "gunzip_single", s, [&] {
            launch_gunzip_single(d.items(), d.list<const uint32_t>(d.at.single_list), n_single, d.list<GzSingle>(d.at.single_res), s);
        });
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(b.sres.data(), d.p + d.at.single_res, sizeof(GzSingle) * n_single, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(ctx, hipStreamSynchronize(s));
    return ZNIPPY_OK;
}

// the decode launch over the non-empty runs; the CRC launch over them and over the first member of every item of the single pass
static int gz_decode_stage(znippy_ctx *ctx, GzBatch &b, const GzDev &d) {
    const uint32_t n_runs = (uint32_t)b.h_runs.size(), n_crc = (uint32_t)b.crc_items.size();
    hipStream_t s = d.s;
    if (n_runs) {
        HIPCHK(ctx, hipMemcpyAsync(d.p + d.at.runs, b.h_runs.data(), sizeof(GzRun) * n_runs, hipMemcpyHostToDevice, s));
        timed(ctx, "gunzip_inflate", s, [&] { launch_gunzip_inflate(d.items(), d.list<const GzRun>(d.at.runs), n_runs, d.list<int32_t>(d.at.run_st), s); });
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(b.run_st.data(), d.p + d.at.run_st, sizeof(int32_t) * n_runs, hipMemcpyDeviceToHost, s));
    }
    if (n_crc) {
        HIPCHK(ctx, hipMemcpyAsync(d.p + d.at.crc_items, b.crc_items.data(), sizeof(InflateItem) * n_crc, hipMemcpyHostToDevice, s));
        HIPCHK(ctx, hipMemsetAsync(d.p + d.at.crc_st, 0, sizeof(int32_t) * n_crc, s));
        timed(ctx, "gunzip_crc", s, [&] {
            launch_inflate_crc(d.list<const InflateItem>(d.at.crc_items), n_crc, d.list<int32_t>(d.at.crc_st), d.list<uint32_t>(d.at.crc_got), s);
        });
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(b.crc_st.data(), d.p + d.at.crc_st, sizeof(int32_t) * n_crc, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipMemcpyAsync(b.crc_got.data(), d.p + d.at.crc_got, sizeof(uint32_t) * n_crc, hipMemcpyDeviceToHost, s));
    }
    if (n_runs || n_crc) HIPCHK(ctx, hipStreamSynchronize(s));
    return ZNIPPY_OK;
}

// The block-start search (znippy_ctx_set_gunzip_cut): the searched items and their chunks up, the slots set to NONE and the count of
// passing positions to 0, the search, slots and count back; what they say goes to the context's statistics
struct GzFindDev {
    uint8_t *p;
    size_t items, chunks, slots, passed, bytes;
};
static GzFindDev gz_find_layout(const gzcut::FindPlan &f) {
    GzFindDev d{};
    auto carve = [&d](size_t sz) { const size_t at = d.bytes; d.bytes += (sz + 15) & ~(size_t)15; return at; };
    d.items = carve(sizeof(gzcut::FindItem) * f.items.size());
    d.chunks = carve(sizeof(gzcut::FindChunk) * f.chunks.size());
    d.slots = carve(sizeof(uint64_t) * f.n_slots);
    d.passed = carve(sizeof(uint64_t));
    return d;
}
static int gz_find_stage(znippy_ctx *ctx, const gzcut::FindPlan &f, const GzFindDev &d, uint64_t cut, std::vector<uint64_t> &slots, hipStream_t s) {
    HIPCHK(ctx, hipMemcpyAsync(d.p + d.items, f.items.data(), sizeof(gzcut::FindItem) * f.items.size(), hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(d.p + d.chunks, f.chunks.data(), sizeof(gzcut::FindChunk) * f.chunks.size(), hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipMemsetAsync(d.p + d.slots, 0xFF, sizeof(uint64_t) * f.n_slots, s));
    HIPCHK(ctx, hipMemsetAsync(d.p + d.passed, 0, sizeof(uint64_t), s));
    timed(ctx, "gunzip_find", s, [&] {
        launch_gunzip_find((const gzcut::FindItem *)(d.p + d.items), (const gzcut::FindChunk *)(d.p + d.chunks), (uint32_t)f.chunks.size(), (uint32_t)cut,
                           (unsigned long long *)(d.p + d.slots), (unsigned long long *)(d.p + d.passed), s);
    });
    HIPCHK(ctx, hipGetLastError());
    slots.resize((size_t)f.n_slots);
    uint64_t passed = 0;
    HIPCHK(ctx, hipMemcpyAsync(slots.data(), d.p + d.slots, sizeof(uint64_t) * f.n_slots, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(&passed, d.p + d.passed, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    ctx->gz_cut_stats[0] = f.tested;
    ctx->gz_cut_stats[1] = passed;
    ctx->gz_cut_stats[2] = gzcut::count_kept(f, slots.data(), cut);
    return ZNIPPY_OK;
}

// The cut at the block starts found (host/gz_cut_plan.h): one more allocation for its lists (entries: a candidate per slot, one per searched
// item and one per entry of its slice of the scan's list at the most, and so records, pieces, groups and CRC entries) and one for the symbols of a pass
struct GzCutDev {
    uint8_t *p;
    size_t cands, stops, recs, pieces, groups, status, crc_items, crc_st, crc_got, resolved, bytes;
    size_t entries;
    uint16_t *scratch;
    uint64_t budget_syms;
};
static GzCutDev gz_cut_layout(const gzcut::FindPlan &f, const GzBatch &b, uint64_t budget_bytes) {
    GzCutDev d{};
    auto carve = [&d](size_t sz) { const size_t at = d.bytes; d.bytes += (sz + 15) & ~(size_t)15; return at; };
    d.entries = (size_t)f.n_slots + f.items.size();
    for (const uint32_t k : f.item_of) d.entries += b.items[k].cand_cap;  // (the scan's member and flush candidates)
    d.cands = carve(sizeof(gzcut::CutCand) * d.entries);
    d.stops = carve(sizeof(uint64_t) * d.entries);
    d.recs = carve(sizeof(gzcut::CutRec) * d.entries);
    d.pieces = carve(sizeof(gzcut::CutPiece) * d.entries);
    d.groups = carve(sizeof(gzcut::CutGroup) * d.entries);
    d.status = carve(sizeof(int32_t) * d.entries);
    d.crc_items = carve(sizeof(InflateItem) * d.entries);
    d.crc_st = carve(sizeof(int32_t) * d.entries);
    d.crc_got = carve(sizeof(uint32_t) * d.entries);
    d.resolved = carve(sizeof(uint64_t) * d.entries);  // per piece
    uint64_t rooms = 0;  // no pass holds more symbols than the searched items have room for
    for (const uint32_t k : f.item_of) rooms += b.items[k].room;
    d.budget_syms = std::max<uint64_t>(1, std::min<uint64_t>(budget_bytes / 2, rooms));
    return d;
}

// Probe, plan, and pass by pass decode, tails and apply; then the CRC of every piece.  Items whose plan stands and whose pieces and
// CRC are clean get their results here (b.cut_done, cut_res); every other item is left to the stages behind, untouched but for bytes
// inside its own room.
struct GzCutResult { uint32_t item; uint32_t members, segments; uint64_t out_len; };
static int gz_cut_stage(znippy_ctx *ctx, GzBatch &b, const GzDev &d, const gzcut::FindPlan &f, const GzCutDev &c, const uint64_t *slots, uint64_t cut,
                        uint64_t seg_min, std::vector<GzCutResult> &done) {
    hipStream_t s = d.s;
    std::vector<gzcut::CutCand> cands;
    std::vector<uint64_t> stops, kept, raw;
    std::vector<std::pair<uint64_t, uint32_t>> all;  // (bit, member) of one item
    std::vector<size_t> first_cand;  // per find item, and one more
    for (size_t fi = 0; fi < f.items.size(); fi++) {
        first_cand.push_back(cands.size());
        gzcut::kept_of(f, fi, slots, cut, kept);
        if (kept.empty()) continue;  // (nothing to cut at that the stages behind do not cut at themselves)
        const uint32_t k = f.item_of[fi];
        all.clear();
        all.emplace_back(0, 1u);
        for (const uint64_t v : kept) all.emplace_back(v, 0u);
        if (b.count[k] && b.count[k] <= b.items[k].cand_cap) {  // the scan's candidates, kept as gz_candidates keeps them
            raw.assign(b.raw.begin() + b.items[k].cand_base, b.raw.begin() + b.items[k].cand_base + b.count[k]);
            const size_t n_kept = gzp::keep_candidates(raw.data(), raw.size(), seg_min);
            for (size_t j = 0; j < n_kept; j++)
                if ((raw[j] >> 1) < b.items[k].src_len) all.emplace_back((raw[j] >> 1) * 8, (uint32_t)(raw[j] & 1));
        }
        std::sort(all.begin(), all.end());
        all.erase(std::unique(all.begin(), all.end()), all.end());
        const uint32_t base = (uint32_t)stops.size();
        for (const auto &c : all)
            if (!c.second) stops.push_back(c.first);
        const uint32_t end = (uint32_t)stops.size();
        uint32_t next_stop = base;  // the first stop behind the position
        for (const auto &c : all) {
            while (next_stop < end && stops[next_stop] <= c.first) next_stop++;
            cands.push_back(gzcut::CutCand{k, c.second, c.first, next_stop, end});
        }
    }
    first_cand.push_back(cands.size());
    if (cands.empty()) return ZNIPPY_OK;
    if (cands.size() > c.entries || stops.size() > c.entries) return ZNIPPY_E_NOMEM;  // (cannot happen: gz_cut_layout counts them)
    const uint32_t n_cands = (uint32_t)cands.size();
    HIPCHK(ctx, hipMemcpyAsync(c.p + c.cands, cands.data(), sizeof(gzcut::CutCand) * n_cands, hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(c.p + c.stops, stops.data(), sizeof(uint64_t) * stops.size(), hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipMemsetAsync(c.p + c.resolved, 0, sizeof(uint64_t) * c.entries, s));
    timed(ctx, "gunzip_cut_probe", s, [&] {
        launch_gunzip_cut_probe(d.items(), (const gzcut::CutCand *)(c.p + c.cands), n_cands, (const uint64_t *)(c.p + c.stops), (gzcut::CutRec *)(c.p + c.recs), s);
    });
    HIPCHK(ctx, hipGetLastError());
    std::vector<gzcut::CutRec> recs(n_cands);
    HIPCHK(ctx, hipMemcpyAsync(recs.data(), c.p + c.recs, sizeof(gzcut::CutRec) * n_cands, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    std::vector<gzcut::CutPiece> pieces;
    std::vector<gzcut::CutItemPlan> plans;
    std::vector<gzcut::CutMember> mems;
    for (size_t fi = 0; fi < f.items.size(); fi++) {
        const size_t c0 = first_cand[fi], c1 = first_cand[fi + 1];
        if (c0 == c1) continue;
        const uint32_t k = f.item_of[fi];
        gzcut::plan_cut(cands.data() + c0, recs.data() + c0, c1 - c0, k, b.items[k].src_len, b.items[k].room, c.budget_syms, pieces, mems, plans);
    }
    if (plans.empty()) return ZNIPPY_OK;
    std::vector<gzcut::CutPass> passes;
    std::vector<gzcut::CutGroup> groups;
    gzcut::make_passes(pieces, c.budget_syms, passes, groups);
    const uint32_t n_pieces = (uint32_t)pieces.size();
    if (pieces.size() > c.entries || groups.size() > c.entries) return ZNIPPY_E_NOMEM;  // (cannot happen: a piece per candidate at the most)
    for (const gzcut::CutPiece &pc : pieces)
        if (pc.marker && (pc.sym_off > c.budget_syms || pc.out_len > c.budget_syms - pc.sym_off)) return ZNIPPY_E_NOMEM;  // (likewise: make_passes places them inside)
    HIPCHK(ctx, hipMemcpyAsync(c.p + c.pieces, pieces.data(), sizeof(gzcut::CutPiece) * n_pieces, hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(c.p + c.groups, groups.data(), sizeof(gzcut::CutGroup) * groups.size(), hipMemcpyHostToDevice, s));
    const gzcut::CutPiece *const d_pieces = (const gzcut::CutPiece *)(c.p + c.pieces);
    unsigned long long *const d_resolved = (unsigned long long *)(c.p + c.resolved);
    for (const gzcut::CutPass &ps : passes) {  // (ordered by the stream: a pass starts from the bytes the passes before it left)
        const uint32_t np = (uint32_t)(ps.piece1 - ps.piece0), ng = (uint32_t)(ps.group1 - ps.group0);
        timed(ctx, "gunzip_decode", s, [&] { launch_gunzip_cut_decode(d.items(), d_pieces + ps.piece0, np, c.scratch, (int32_t *)(c.p + c.status) + ps.piece0, s); });
        HIPCHK(ctx, hipGetLastError());
        timed(ctx, "gunzip_tails", s, [&] { launch_gunzip_cut_tails(d.items(), d_pieces, (const gzcut::CutGroup *)(c.p + c.groups) + ps.group0, ng, c.scratch, d_resolved, s); });
        HIPCHK(ctx, hipGetLastError());
        timed(ctx, "gunzip_apply", s, [&] { launch_gunzip_cut_apply(d.items(), d_pieces + ps.piece0, np, c.scratch, d_resolved + ps.piece0, s); });
        HIPCHK(ctx, hipGetLastError());
    }
    // the CRC of every non-empty piece, combined per item on the host
    std::vector<InflateItem> crc_items;
    std::vector<size_t> crc_of(pieces.size(), (size_t)-1);
    for (size_t p = 0; p < pieces.size(); p++) {
        if (!pieces[p].out_len) continue;
        InflateItem it;
        it.src = nullptr; it.dst = b.items[pieces[p].item].dst + pieces[p].out_off; it.src_len = 0; it.out_len = pieces[p].out_len;
        it.method = 8; it.want_crc = 0; it.has_crc = 0; it.pad = 0;
        crc_of[p] = crc_items.size();
        crc_items.push_back(it);
    }
    const uint32_t n_crc = (uint32_t)crc_items.size();
    std::vector<int32_t> piece_st(n_pieces);
    std::vector<uint32_t> crc_got(n_crc);
    std::vector<uint64_t> resolved(n_pieces);
    if (n_crc) {
        HIPCHK(ctx, hipMemcpyAsync(c.p + c.crc_items, crc_items.data(), sizeof(InflateItem) * n_crc, hipMemcpyHostToDevice, s));
        HIPCHK(ctx, hipMemsetAsync(c.p + c.crc_st, 0, sizeof(int32_t) * n_crc, s));
        timed(ctx, "gunzip_cut_crc", s, [&] { launch_inflate_crc((const InflateItem *)(c.p + c.crc_items), n_crc, (int32_t *)(c.p + c.crc_st), (uint32_t *)(c.p + c.crc_got), s); });
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(crc_got.data(), c.p + c.crc_got, sizeof(uint32_t) * n_crc, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(ctx, hipMemcpyAsync(piece_st.data(), c.p + c.status, sizeof(int32_t) * n_pieces, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(resolved.data(), c.p + c.resolved, sizeof(uint64_t) * n_pieces, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    b.cut_done.assign(b.items.size(), 0);
    for (const gzcut::CutItemPlan &pl : plans) {
        bool ok = true;
        for (size_t p = pl.piece0; p < pl.piece1; p++)
            if (piece_st[p] != 0) ok = false;
        for (size_t m = pl.member0; m < pl.member1 && ok; m++) {
            uint32_t crc = 0;
            for (size_t p = mems[m].piece0; p < mems[m].piece1; p++)
                if (pieces[p].out_len) crc = gzp::crc32_combine(crc, crc_got[crc_of[p]], pieces[p].out_len);
            if (crc != mems[m].crc) ok = false;
        }
        if (!ok) continue;  // (the stages behind decode the item again and say what it is)
        b.cut_done[pl.item] = 1;
        done.push_back(GzCutResult{pl.item, pl.members, (uint32_t)(pl.piece1 - pl.piece0), pl.out_len});
        ctx->gz_cut_stats[3] += pl.piece1 - pl.piece0 - pl.members;
        for (size_t p = pl.piece0; p < pl.piece1; p++) {
            ctx->gz_cut_stats[pieces[p].marker ? 4 : 5]++;
            ctx->gz_cut_stats[6] += resolved[p];
        }
    }
    ctx->gz_cut_stats[7] = passes.size();
    return ZNIPPY_OK;
}

static int gunzip_batch(znippy_ctx *ctx, const void *d_src, uint64_t src_cap, const uint64_t *src_off, const uint64_t *src_len, uint64_t n, void *d_out,
                        uint64_t out_cap, const uint64_t *out_off, const uint64_t *out_room, uint64_t seg_min, uint64_t *out_len, int32_t *status,
                        uint32_t *members, uint32_t *segments) {
    if (!ctx_enter(ctx)) return ZNIPPY_E_INVAL;
    if (!ctx || n >= 0xFFFFFFF0ull) return ZNIPPY_E_INVAL;
    if (!n) return ZNIPPY_OK;
    if (!src_off || !src_len || !out_room || !out_len || !d_src || (out_cap && !d_out)) return ZNIPPY_E_INVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ctx->n_ktimes = 0;
    memset(ctx->gz_cut_stats, 0, sizeof ctx->gz_cut_stats);
    { const int prc = poison_enter(ctx); if (prc) return prc; }
    if (!seg_min) {
        seg_min = gzp::SEG_MIN_DEFAULT;
        if (const char *e = getenv("ZNIPPY_GZ_SEG_MIN")) {
            const unsigned long long v = strtoull(e, nullptr, 10);
            if (v) seg_min = v;
        }
    }

    const GzCall call{(const uint8_t *)d_src, src_cap, src_off, src_len, n, (uint8_t *)d_out, out_cap, out_off, out_room, seg_min, out_len, members, segments};
    GzBatch b;
    int rc;
    if ((rc = gz_admit(call, b))) return rc;
    if (!b.items.empty()) {
        struct Guard {
            znippy_ctx *ctx;
            uint8_t *p = nullptr, *find = nullptr, *cut = nullptr;
            uint16_t *syms = nullptr;
            ~Guard() { tfree(ctx, p); tfree(ctx, find); tfree(ctx, cut); tfree(ctx, syms); }
        } g{ctx};
        const uint64_t cut = ctx->gz_cut;
        gzcut::FindPlan fp;
        if (cut && gzcut::find_plan(b.items.data(), b.items.size(), cut, fp) != gzcut::OK) fp = gzcut::FindPlan{};  // (beyond the slot limit: as with the value 0)
        GzFindDev fd = gz_find_layout(fp);
        const GzLayout at = gz_layout(b);
        HIPCHK(ctx, tmalloc(ctx, &g.p, at.bytes));
        GzCutDev cd{};
        if (!fp.items.empty()) {
            uint64_t budget = 1024ull << 20;
            if (const char *e = getenv("ZNIPPY_GZ_CUT_SCRATCH_MB")) {
                const unsigned long long v = strtoull(e, nullptr, 10);
                if (v) budget = std::min<unsigned long long>(v, 1ull << 20) << 20;
            }
            cd = gz_cut_layout(fp, b, budget);
            // (memory the value 0 does not take: where the device has none left for it, the call runs as with the value 0)
            if (tmalloc(ctx, &g.find, fd.bytes) != hipSuccess || tmalloc(ctx, &g.cut, cd.bytes) != hipSuccess ||
                tmalloc(ctx, &g.syms, (size_t)cd.budget_syms * 2) != hipSuccess) {
                (void)hipGetLastError();
                fp = gzcut::FindPlan{};
            }
        }
        fd.p = g.find;
        cd.p = g.cut;
        cd.scratch = g.syms;
        const GzDev d{g.p, at, ctx->stream};
        if ((rc = gz_scan_stage(ctx, b, d))) return rc;
        std::vector<uint64_t> cut_slots;
        std::vector<GzCutResult> cut_res;
        if (!fp.items.empty() && (rc = gz_find_stage(ctx, fp, fd, cut, cut_slots, ctx->stream))) return rc;
        if (!fp.items.empty() && (rc = gz_cut_stage(ctx, b, d, fp, cd, cut_slots.data(), cut, seg_min, cut_res))) return rc;
        if ((rc = gz_candidates(b, seg_min))) return rc;
        if ((rc = gz_probe_stage(ctx, b, d))) return rc;
        if ((rc = gz_decode_plan(b))) return rc;
        if ((rc = gz_decode_stage(ctx, b, d))) return rc;
        gz_verdict(call, b);
        for (const GzCutResult &r : cut_res) {  // (status 0, as gz_admit left it)
            const uint32_t i = b.item_of[r.item];
            out_len[i] = r.out_len;
            if (members) members[i] = r.members;
            if (segments) segments[i] = r.segments;
        }
    }
    if (status) memcpy(status, b.st.data(), sizeof(int32_t) * n);
    return ZNIPPY_OK;
}

extern "C" int znippy_gunzip_batch(znippy_ctx *ctx, const void *d_src, uint64_t src_cap, const uint64_t *src_off, const uint64_t *src_len, uint64_t n,
                                   void *d_out, uint64_t out_cap, const uint64_t *out_off, const uint64_t *out_room, uint64_t seg_min, uint64_t *out_len,
                                   int32_t *status, uint32_t *members, uint32_t *segments) {
    ZN_NO_THROW(gunzip_batch(ctx, d_src, src_cap, src_off, src_len, n, d_out, out_cap, out_off, out_room, seg_min, out_len, status, members, segments))
}

// ---- whole bzip2 files (znippy_bunzip2_batch) ---------------------------------------------------------
// The items that pass bz_admit are scanned for block magics; bz_start sorts the candidates into the items' chains; then passes of at
// most n_slots jobs: bzp::choose names them, decode and walk leave a record each, bzp::advance walks the chains over the records,
// and the blocks landed on are expanded into the rooms and checksummed (not in measure mode) before the next pass reuses the slots.
// Two device allocations, both sized from the source lengths and the slot count and made before anything is queued: the lists, and
// the slots.
static_assert(BZ_OK == ZNIPPY_OK && BZ_E_INVAL == ZNIPPY_E_INVAL && BZ_E_NOMEM == ZNIPPY_E_NOMEM && BZ_E_DST_SMALL == ZNIPPY_E_DST_SMALL &&
              BZ_E_CORRUPT == ZNIPPY_E_CORRUPT && BZ_E_UNSUPPORTED == ZNIPPY_E_UNSUPPORTED && BZ_E_CHECKSUM == ZNIPPY_E_CHECKSUM,
              "host/bz_plan.h gives out the codes of znippy_hip.h");

struct BzDev {  // the list allocation and where its lists are, and the slots
    uint8_t *p;
    size_t items, chunks, count, raw, jobs, recs, lands, crc, bytes;
    size_t jobs_cap, n_slots;  // entries of jobs and recs; of lands, crc and the slots
    uint8_t *slots;
    template <typename T>
    T *list(size_t off) const { return (T *)(p + off); }
};

static int bz_scan_stage(znippy_ctx *ctx, BzBatch &b, const BzDev &d, hipStream_t s) {
    HIPCHK(ctx, hipMemcpyAsync(d.p + d.items, b.items.data(), sizeof(BzItem) * b.items.size(), hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(d.p + d.chunks, b.chunks.data(), sizeof(BzChunk) * b.chunks.size(), hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipMemsetAsync(d.p + d.count, 0, 16, s));
    timed(ctx, "bunzip2_scan", s, [&] {
        launch_bunzip2_scan(d.list<const BzItem>(d.items), d.list<const BzChunk>(d.chunks), (uint32_t)b.chunks.size(), d.list<uint32_t>(d.count),
                            d.list<uint64_t>(d.raw), (uint32_t)b.cand_total, s);
    });
    HIPCHK(ctx, hipGetLastError());
    uint32_t count = 0;
    HIPCHK(ctx, hipMemcpyAsync(&count, d.p + d.count, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    const size_t n_raw = (size_t)std::min<uint64_t>(count, b.cand_total);
    b.raw.resize(n_raw);
    if (n_raw) {
        HIPCHK(ctx, hipMemcpyAsync(b.raw.data(), d.p + d.raw, sizeof(uint64_t) * n_raw, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
    }
    bz_start(b, n_raw);
    return ZNIPPY_OK;
}

// one pass: the jobs up, decode and walk, the records back; the chains; what landed expanded and checksummed
static int bz_pass(znippy_ctx *ctx, BzBatch &b, const BzDev &d, uint32_t split, hipStream_t s) {
    const uint32_t n_jobs = (uint32_t)b.jobs.size();
    if (b.jobs.size() > d.jobs_cap) return ZNIPPY_E_NOMEM;  // (cannot happen: bzp::choose gives out n_slots block jobs and a header job per item at the most)
    for (const BzJob &j : b.jobs)
        if (j.slot >= d.n_slots) return ZNIPPY_E_NOMEM;     // (likewise)
    HIPCHK(ctx, hipMemcpyAsync(d.p + d.jobs, b.jobs.data(), sizeof(BzJob) * n_jobs, hipMemcpyHostToDevice, s));
    timed(ctx, "bunzip2_decode", s, [&] { launch_bunzip2_decode(d.list<const BzItem>(d.items), d.list<const BzJob>(d.jobs), n_jobs, d.list<BzRec>(d.recs), d.slots, s); });
    HIPCHK(ctx, hipGetLastError());
    timed(ctx, "bunzip2_walk", s, [&] { launch_bunzip2_walk(d.list<const BzJob>(d.jobs), n_jobs, d.list<BzRec>(d.recs), d.slots, split, s); });
    HIPCHK(ctx, hipGetLastError());
    b.recs.resize(n_jobs);
    HIPCHK(ctx, hipMemcpyAsync(b.recs.data(), d.p + d.recs, sizeof(BzRec) * n_jobs, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    b.lands.clear();
    bzp::advance(b.chains, b.jobs, b.first_job, b.recs.data(), b.lands);
    const uint32_t n_lands = (uint32_t)b.lands.size();
    if (n_lands > d.n_slots) return ZNIPPY_E_NOMEM;  // (cannot happen: a chain lands on a block job of the pass at most once)
    if (n_lands) {  // (never in measure mode)
        HIPCHK(ctx, hipMemcpyAsync(d.p + d.lands, b.lands.data(), sizeof(BzLand) * n_lands, hipMemcpyHostToDevice, s));
        timed(ctx, "bunzip2_expand", s, [&] { launch_bunzip2_expand(d.list<const BzItem>(d.items), d.list<const BzLand>(d.lands), n_lands, d.slots, s); });
        HIPCHK(ctx, hipGetLastError());
        timed(ctx, "bunzip2_crc", s, [&] { launch_bunzip2_crc(d.list<const BzItem>(d.items), d.list<const BzLand>(d.lands), n_lands, d.list<uint32_t>(d.crc), s); });
        HIPCHK(ctx, hipGetLastError());
        b.got_crc.resize(n_lands);
        HIPCHK(ctx, hipMemcpyAsync(b.got_crc.data(), d.p + d.crc, sizeof(uint32_t) * n_lands, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
        bzp::fold_crc(b.chains, b.lands, b.got_crc.data());
    }
    return ZNIPPY_OK;
}

static int bunzip2_batch(znippy_ctx *ctx, const void *d_src, uint64_t src_cap, const uint64_t *src_off, const uint64_t *src_len, uint64_t n, void *d_out,
                         uint64_t out_cap, const uint64_t *out_off, const uint64_t *out_room, uint64_t slot_cap, uint64_t *out_len, int32_t *status,
                         uint32_t *streams, uint32_t *blocks) {
    if (!ctx_enter(ctx)) return ZNIPPY_E_INVAL;
    if (!ctx || n >= 0xFFFFFFF0ull) return ZNIPPY_E_INVAL;
    if (!n) return ZNIPPY_OK;
    const bool measure = !d_out && !out_cap;
    if (!src_off || !src_len || (!measure && !out_room) || !out_len || !d_src || (out_cap && !d_out)) return ZNIPPY_E_INVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ctx->n_ktimes = 0;
    { const int prc = poison_enter(ctx); if (prc) return prc; }
    uint64_t budget = BZ_SCRATCH_DEFAULT;
    if (const char *e = getenv("ZNIPPY_BZ_SCRATCH_MB")) {
        const unsigned long long v = strtoull(e, nullptr, 10);
        if (v) budget = std::min<unsigned long long>(v, 1ull << 30) << 20;
    }
    uint32_t split = BZ_SPLIT_DEFAULT;
    if (const char *e = getenv("ZNIPPY_BZ_SPLIT")) {
        const unsigned long long v = strtoull(e, nullptr, 10);
        if (v) split = (uint32_t)std::min<unsigned long long>(v, 0xFFFFFFFFull);
    }

    const BzCall call{(const uint8_t *)d_src, src_cap, src_off, src_len, n, (uint8_t *)d_out, out_cap, out_off, out_room, out_len, streams, blocks};
    BzBatch b;
    int rc;
    if ((rc = bz_admit(call, b))) return rc;
    if (!b.items.empty()) {
        const size_t n_slots = bz_slots(b, slot_cap, budget);
        if (!n_slots) return ZNIPPY_E_NOMEM;  // not one slot fits the budget: nothing has been queued
        struct Guard {
            znippy_ctx *ctx;
            uint8_t *p = nullptr, *slots = nullptr;
            ~Guard() { tfree(ctx, p); tfree(ctx, slots); }
        } g{ctx};
        BzDev d{};
        auto carve = [&d](size_t sz) { const size_t at = d.bytes; d.bytes += (sz + 15) & ~(size_t)15; return at; };
        d.items = carve(sizeof(BzItem) * b.items.size());
        d.chunks = carve(sizeof(BzChunk) * b.chunks.size());
        d.count = carve(16);
        d.raw = carve(sizeof(uint64_t) * b.cand_total);
        d.jobs_cap = bz_jobs_max(b, n_slots);
        d.jobs = carve(sizeof(BzJob) * d.jobs_cap);
        d.recs = carve(sizeof(BzRec) * d.jobs_cap);
        d.lands = carve(sizeof(BzLand) * n_slots);
        d.crc = carve(sizeof(uint32_t) * n_slots);
        HIPCHK(ctx, tmalloc(ctx, &g.p, d.bytes));
        HIPCHK(ctx, tmalloc(ctx, &g.slots, n_slots * BZ_SLOT_BYTES));
        d.p = g.p;
        d.slots = g.slots;
        d.n_slots = n_slots;
        hipStream_t s = ctx->stream;
        if ((rc = bz_scan_stage(ctx, b, d, s))) return rc;
        while (bzp::choose(b.chains, n_slots, b.jobs, b.first_job))
            if ((rc = bz_pass(ctx, b, d, split, s))) return rc;
        bz_verdict(call, b);
    }
    if (status) memcpy(status, b.st.data(), sizeof(int32_t) * n);
    return ZNIPPY_OK;
}

extern "C" int znippy_bunzip2_batch(znippy_ctx *ctx, const void *d_src, uint64_t src_cap, const uint64_t *src_off, const uint64_t *src_len, uint64_t n,
                                    void *d_out, uint64_t out_cap, const uint64_t *out_off, const uint64_t *out_room, uint64_t slot_cap, uint64_t *out_len,
                                    int32_t *status, uint32_t *streams, uint32_t *blocks) {
    ZN_NO_THROW(bunzip2_batch(ctx, d_src, src_cap, src_off, src_len, n, d_out, out_cap, out_off, out_room, slot_cap, out_len, status, streams, blocks))
}

// ---- the members of tars (znippy_tar_list_batch) -------------------------------------------------------
// The items that pass tl_admit are scanned block by block, the chains from their first blocks are marked in tl_rounds rounds, and
// the marked members are judged and counted; tl_place turns the totals into statuses and room; the write launch leaves records and
// names in staging lists, which tl_accept checks record by record on their way to the caller; the gather moves the contents.  One
// device allocation (tl_layout) and the staging lists, all sized from the item lengths and the caps and made before anything is queued.
static_assert(TL_OK == ZNIPPY_OK && TL_E_INVAL == ZNIPPY_E_INVAL && TL_E_NOMEM == ZNIPPY_E_NOMEM && TL_E_DST_SMALL == ZNIPPY_E_DST_SMALL &&
              TL_E_CORRUPT == ZNIPPY_E_CORRUPT && TL_E_UNSUPPORTED == ZNIPPY_E_UNSUPPORTED, "host/tar_list_plan.h gives out the codes of znippy_hip.h");

static int tar_list_batch(znippy_ctx *ctx, const void *d_tar, uint64_t tar_cap, const uint64_t *tar_off, const uint64_t *tar_len, uint64_t n,
                          const char *name_prefix, uint64_t prefix_len, const char *name_suffix, uint64_t suffix_len, znippy_tar_member *members,
                          uint64_t members_cap, char *names, uint64_t names_cap, void *d_out, uint64_t out_cap, uint64_t *member_first,
                          uint64_t *names_bytes, uint64_t *out_bytes, int32_t *status) {
    if (!ctx_enter(ctx)) return ZNIPPY_E_INVAL;
    if (!ctx || n >= 0xFFFFFFF0ull) return ZNIPPY_E_INVAL;
    if (!member_first || !names_bytes || !out_bytes || (prefix_len && !name_prefix) || (suffix_len && !name_suffix) || prefix_len >= TL_FILTER_MAX ||
        suffix_len >= TL_FILTER_MAX || (members_cap && !members) || (names_cap && !names) || (out_cap && !d_out))
        return ZNIPPY_E_INVAL;
    const bool measure = !members;
    if (measure && (names || d_out)) return ZNIPPY_E_INVAL;
    if (!n) { member_first[0] = 0; *names_bytes = *out_bytes = 0; return ZNIPPY_OK; }
    if (!tar_off || !tar_len || !d_tar) return ZNIPPY_E_INVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    ctx->n_ktimes = 0;
    { const int prc = poison_enter(ctx); if (prc) return prc; }

    const TlCall call{(const uint8_t *)d_tar, tar_cap, tar_off, tar_len, n, members, members_cap, names, names_cap, (uint8_t *)d_out, out_cap,
                      member_first, names_bytes, out_bytes};
    TlBatch b;
    int rc;
    if ((rc = tl_admit(call, b))) return rc;
    const uint32_t n_items = (uint32_t)b.items.size(), n_chunks = (uint32_t)b.chunks.size(), n_nodes = (uint32_t)b.n_nodes;
    if (n_items) {
        struct Guard {
            znippy_ctx *ctx;
            uint8_t *p = nullptr; znippy_tar_member *recs = nullptr; char *names = nullptr; RangePiece *pieces = nullptr;
            ~Guard() { tfree(ctx, p); tfree(ctx, recs); tfree(ctx, names); tfree(ctx, pieces); }
        } g{ctx};
        const TlLayout at = tl_layout(b, prefix_len + suffix_len);
        size_t cap_recs, cap_names, cap_pieces;
        if ((rc = tl_staging(call, b, &cap_recs, &cap_names, &cap_pieces))) return rc;
        std::vector<uint8_t> filter(prefix_len + suffix_len + 16, 0);
        if (prefix_len) memcpy(filter.data(), name_prefix, prefix_len);
        if (suffix_len) memcpy(filter.data() + prefix_len, name_suffix, suffix_len);
        std::vector<znippy_tar_member> h_recs;
        std::vector<char> h_names;
        // every allocation, then the stream
        HIPCHK(ctx, tmalloc(ctx, &g.p, at.bytes));
        if (!measure) {
            HIPCHK(ctx, tmalloc(ctx, &g.recs, sizeof(znippy_tar_member) * cap_recs));
            HIPCHK(ctx, tmalloc(ctx, &g.names, cap_names));
            if (cap_pieces) HIPCHK(ctx, tmalloc(ctx, &g.pieces, sizeof(RangePiece) * cap_pieces));
            h_recs.resize(cap_recs);
            h_names.resize(cap_names);
        }
        auto list = [&g](size_t off) { return g.p + off; };
        const TlItem *d_items = (const TlItem *)list(at.items);
        const TlChunk *d_chunks = (const TlChunk *)list(at.chunks);
        TlNode *d_nodes = (TlNode *)list(at.nodes);
        uint32_t *jump[2] = {(uint32_t *)list(at.jump_a), (uint32_t *)list(at.jump_b)};
        HIPCHK(ctx, hipMemcpyAsync(list(at.items), b.items.data(), sizeof(TlItem) * n_items, hipMemcpyHostToDevice, s));
        HIPCHK(ctx, hipMemcpyAsync(list(at.chunks), b.chunks.data(), sizeof(TlChunk) * n_chunks, hipMemcpyHostToDevice, s));
        HIPCHK(ctx, hipMemcpyAsync(list(at.filter), filter.data(), filter.size(), hipMemcpyHostToDevice, s));
        HIPCHK(ctx, hipMemsetAsync(list(at.totals), 0xFF, sizeof(TlTotal) * n_items, s));  // the keys: TL_KEY_NONE
        timed(ctx, "tar_scan", s, [&] { launch_tar_scan(d_items, d_chunks, n_chunks, d_nodes, list(at.mark), jump[0], s); });
        HIPCHK(ctx, hipGetLastError());
        const uint32_t rounds = tl_rounds(b.max_nodes);
        timed(ctx, "tar_chain", s, [&] {
            for (uint32_t r = 0; r < rounds; r++) launch_tar_chain(jump[r & 1], jump[~r & 1], list(at.mark), n_nodes, s);
        });
        HIPCHK(ctx, hipGetLastError());
        timed(ctx, "tar_emit", s, [&] {
            launch_tar_emit(d_items, n_items, d_chunks, n_chunks, d_nodes, list(at.mark), (uint32_t *)list(at.pred), n_nodes, list(at.filter), (uint32_t)prefix_len,
                            (uint32_t)suffix_len, (uint32_t *)list(at.pick), (uint32_t *)list(at.src), (TlSum *)list(at.sums), (TlTotal *)list(at.totals), s);
        });
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(b.totals.data(), list(at.totals), sizeof(TlTotal) * n_items, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
        tl_place(call, b);
        if (!measure && b.take_members) {
            if (b.take_members > cap_recs || b.take_names > cap_names) return ZNIPPY_E_NOMEM;  // (cannot happen: tl_place keeps to the caps and the item sizes)
            HIPCHK(ctx, hipMemcpyAsync(list(at.bases), b.bases.data(), sizeof(TlBase) * n_items, hipMemcpyHostToDevice, s));
            timed(ctx, "tar_emit_write", s, [&] {
                launch_tar_emit_write(d_items, d_chunks, n_chunks, d_nodes, (const uint32_t *)list(at.pick), (const uint32_t *)list(at.src),
                                      (const TlSum *)list(at.sums), (const TlBase *)list(at.bases), g.recs, b.take_members, g.names, b.take_names, s);
            });
            HIPCHK(ctx, hipGetLastError());
            HIPCHK(ctx, hipMemcpyAsync(h_recs.data(), g.recs, sizeof(znippy_tar_member) * b.take_members, hipMemcpyDeviceToHost, s));
            if (b.take_names) HIPCHK(ctx, hipMemcpyAsync(h_names.data(), g.names, b.take_names, hipMemcpyDeviceToHost, s));
            HIPCHK(ctx, hipStreamSynchronize(s));
            tl_accept(call, b, h_recs.data(), b.take_members, h_names.data(), b.take_names);
            if (!b.pieces.empty()) {
                if (b.pieces.size() > cap_pieces) return ZNIPPY_E_NOMEM;  // (cannot happen: tl_staging counts them)
                HIPCHK(ctx, hipMemcpyAsync(g.pieces, b.pieces.data(), sizeof(RangePiece) * b.pieces.size(), hipMemcpyHostToDevice, s));
                timed(ctx, "tar_gather", s, [&] { launch_range_gather(g.pieces, (uint32_t)b.pieces.size(), s); });
                HIPCHK(ctx, hipGetLastError());
                HIPCHK(ctx, hipStreamSynchronize(s));
            }
        }
    }
    if (status) memcpy(status, b.st.data(), sizeof(int32_t) * n);
    return ZNIPPY_OK;
}

extern "C" int znippy_tar_list_batch(znippy_ctx *ctx, const void *d_tar, uint64_t tar_cap, const uint64_t *tar_off, const uint64_t *tar_len, uint64_t n,
                                     const char *name_prefix, uint64_t prefix_len, const char *name_suffix, uint64_t suffix_len,
                                     znippy_tar_member *members, uint64_t members_cap, char *names, uint64_t names_cap, void *d_out, uint64_t out_cap,
                                     uint64_t *member_first, uint64_t *names_bytes, uint64_t *out_bytes, int32_t *status) {
    ZN_NO_THROW(tar_list_batch(ctx, d_tar, tar_cap, tar_off, tar_len, n, name_prefix, prefix_len, name_suffix, suffix_len, members, members_cap, names,
                               names_cap, d_out, out_cap, member_first, names_bytes, out_bytes, status))
}

// ---- whole xz files (znippy_unxz_batch) ----------------------------------------------------------------
// The items that pass xz_admit are walked from their ends: a round brings the byte ranges the walks ask for to the host
// (xz_wants, the tail launch, one copy back, xz_give) until every walk is done — one round for one-stream files whose footer and
// index lie in the last XZ_TAIL bytes.  xz_plan_jobs then knows every block; one decode launch and one check launch serve them
// all, and xz_verdict judges the records.  Device memory: the tail stage's lists and staging buffer, sized from the item count
// and the first round's ranges and made before the first stream operation (a later round that asks for more, a long index,
// gets a larger staging buffer: never more than the source bytes); the job lists, whose size only the walk gives, once the rounds
// are over and the stream is idle.
static_assert(XZ_OK == ZNIPPY_OK && XZ_E_INVAL == ZNIPPY_E_INVAL && XZ_E_NOMEM == ZNIPPY_E_NOMEM && XZ_E_DST_SMALL == ZNIPPY_E_DST_SMALL &&
              XZ_E_CORRUPT == ZNIPPY_E_CORRUPT && XZ_E_UNSUPPORTED == ZNIPPY_E_UNSUPPORTED && XZ_E_CHECKSUM == ZNIPPY_E_CHECKSUM,
              "host/xz_plan.h gives out the codes of znippy_hip.h");

static int unxz_batch(znippy_ctx *ctx, const void *d_src, uint64_t src_cap, const uint64_t *src_off, const uint64_t *src_len, uint64_t n, void *d_out,
                      uint64_t out_cap, const uint64_t *out_off, const uint64_t *out_room, uint64_t *out_len, int32_t *status, uint32_t *streams,
                      uint32_t *blocks, uint32_t *unverified) {
    if (!ctx_enter(ctx)) return ZNIPPY_E_INVAL;
    if (!ctx || n >= 0xFFFFFFF0ull) return ZNIPPY_E_INVAL;
    if (!n) return ZNIPPY_OK;
    const bool measure = !d_out && !out_cap;
    if (!src_off || !src_len || (!measure && !out_room) || !out_len || !d_src || (out_cap && !d_out)) return ZNIPPY_E_INVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ctx->n_ktimes = 0;
    { const int prc = poison_enter(ctx); if (prc) return prc; }

    const XzCall call{(const uint8_t *)d_src, src_cap, src_off, src_len, n, (uint8_t *)d_out, out_cap, out_off, out_room, out_len, streams, blocks, unverified};
    XzBatch b;
    int rc;
    if ((rc = xz_admit(call, b))) return rc;
    if (!b.items.empty()) {
        struct Guard {
            znippy_ctx *ctx;
            uint8_t *lists = nullptr, *stage = nullptr, *jobs = nullptr;
            ~Guard() { tfree(ctx, lists); tfree(ctx, stage); tfree(ctx, jobs); }
        } g{ctx};
        hipStream_t s = ctx->stream;
        const size_t n_items = b.items.size();
        const size_t items_bytes = (sizeof(XzItem) * n_items + 15) & ~(size_t)15;
        uint64_t need = xz_wants(b), stage_cap = need;
        HIPCHK(ctx, tmalloc(ctx, &g.lists, items_bytes + 2 * sizeof(XzRange) * n_items));
        HIPCHK(ctx, tmalloc(ctx, &g.stage, (size_t)stage_cap));
        const XzItem *d_items = (const XzItem *)g.lists;
        XzRange *d_ranges = (XzRange *)(g.lists + items_bytes);
        HIPCHK(ctx, hipMemcpyAsync(g.lists, b.items.data(), sizeof(XzItem) * n_items, hipMemcpyHostToDevice, s));
        while (need) {
            if (need > stage_cap) {  // (the stream is idle: the round before ended with a wait)
                tfree(ctx, g.stage);
                g.stage = nullptr;
                HIPCHK(ctx, tmalloc(ctx, &g.stage, (size_t)need));
                stage_cap = need;
            }
            const uint32_t n_ranges = (uint32_t)b.ranges.size();  // (at most two per item)
            HIPCHK(ctx, hipMemcpyAsync(d_ranges, b.ranges.data(), sizeof(XzRange) * n_ranges, hipMemcpyHostToDevice, s));
            timed(ctx, "unxz_tail", s, [&] { launch_unxz_tail(d_items, d_ranges, n_ranges, g.stage, s); });
            HIPCHK(ctx, hipGetLastError());
            b.stage.resize((size_t)need);
            HIPCHK(ctx, hipMemcpyAsync(b.stage.data(), g.stage, (size_t)need, hipMemcpyDeviceToHost, s));
            HIPCHK(ctx, hipStreamSynchronize(s));
            xz_give(b);
            need = xz_wants(b);
        }
        if ((rc = xz_plan_jobs(call, b))) return rc;
        const size_t n_jobs = b.jobs.size();
        if (n_jobs) {  // (never in measure mode)
            const size_t jobs_bytes = (sizeof(XzJob) * n_jobs + 15) & ~(size_t)15, recs_bytes = sizeof(XzRec) * n_jobs;
            HIPCHK(ctx, tmalloc(ctx, &g.jobs, jobs_bytes + recs_bytes + sizeof(uint64_t) * n_jobs));
            const XzJob *d_jobs = (const XzJob *)g.jobs;
            XzRec *d_recs = (XzRec *)(g.jobs + jobs_bytes);
            uint64_t *d_sums = (uint64_t *)(g.jobs + jobs_bytes + recs_bytes);
            HIPCHK(ctx, hipMemcpyAsync(g.jobs, b.jobs.data(), sizeof(XzJob) * n_jobs, hipMemcpyHostToDevice, s));
            timed(ctx, "unxz_decode", s, [&] { launch_unxz_decode(d_items, d_jobs, (uint32_t)n_jobs, d_recs, s); });
            HIPCHK(ctx, hipGetLastError());
            timed(ctx, "unxz_check", s, [&] { launch_unxz_check(d_items, d_jobs, (uint32_t)n_jobs, d_sums, s); });
            HIPCHK(ctx, hipGetLastError());
            b.recs.resize(n_jobs);
            b.sums.resize(n_jobs);
            HIPCHK(ctx, hipMemcpyAsync(b.recs.data(), d_recs, recs_bytes, hipMemcpyDeviceToHost, s));
            HIPCHK(ctx, hipMemcpyAsync(b.sums.data(), d_sums, sizeof(uint64_t) * n_jobs, hipMemcpyDeviceToHost, s));
            HIPCHK(ctx, hipStreamSynchronize(s));
        }
        xz_verdict(call, b);
    }
    if (status) memcpy(status, b.st.data(), sizeof(int32_t) * n);
    return ZNIPPY_OK;
}

extern "C" int znippy_unxz_batch(znippy_ctx *ctx, const void *d_src, uint64_t src_cap, const uint64_t *src_off, const uint64_t *src_len, uint64_t n,
                                 void *d_out, uint64_t out_cap, const uint64_t *out_off, const uint64_t *out_room, uint64_t *out_len, int32_t *status,
                                 uint32_t *streams, uint32_t *blocks, uint32_t *unverified) {
    ZN_NO_THROW(unxz_batch(ctx, d_src, src_cap, src_off, src_len, n, d_out, out_cap, out_off, out_room, out_len, status, streams, blocks, unverified))
}
