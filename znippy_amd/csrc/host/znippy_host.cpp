// Compiled host side of the Znippy hot path (include/znippy_host.h): the reference's pipeline entry
// points restated in C++17 over the device C ABI (include/znippy_hip.h).  What runs here is host
// plumbing only — chunking rules, staging, file I/O, index/manifest/footer serialisation, report
// arithmetic; every byte of codec/hash work goes through libznippy_hip's kernels.
#include "../../../include/znippy_host.h"
#include "../../../include/znippy_hip.h"
#include "arrow_ipc.h"
#include "read_plan.h"
#include "zip_dir.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <deque>
#include <dirent.h>
#include <mutex>
#include <cstdio>
#include <cstring>
#include <fcntl.h>
#include <functional>
#include <map>
#include <memory>
#include <sched.h>
#include <string>
#include <sys/stat.h>
#include <thread>
#include <unistd.h>
#include <unordered_map>
#include <unordered_set>
#include <vector>

namespace {

thread_local std::string g_err;
int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

constexpr uint64_t SLICE_SIZE = 8ull * 1024 * 1024;  // stream_packer.rs:L31
constexpr uint64_t SLOT_SIZE = 200ull * 1024 * 1024;  // slot_packer.rs:L30
constexpr int N_STAGE = 3;                            // pinned staging slots in flight on the write side
constexpr size_t MAX_SLOT_ROUNDS = 1u << 20;

uint64_t env_mb(const char *name, uint64_t dflt_mb) {
    const char *v = getenv(name);
    const uint64_t mb = v && *v ? strtoull(v, nullptr, 10) : 0;
    return (mb ? mb : dflt_mb) << 20;
}
// Bytes per GPU hand-off: one pinned staging slot on the write side, one decoded range on the read side.
uint64_t stage_bytes() { return env_mb("ZNIPPY_HOST_SLOT_MB", 128); }
uint64_t range_bytes(bool save) { return env_mb("ZNIPPY_HOST_RANGE_MB", save ? 256 : 1024); }
// Write side, opt-in: every blob_offset of the archive is a multiple of this power of two (1 .. 4096; anything else: 1).
uint32_t blob_align() {
    const char *v = getenv("ZNIPPY_HOST_BLOB_ALIGN");
    const unsigned long a = v && *v ? strtoul(v, nullptr, 10) : 1;
    return a >= 1 && a <= 4096 && !(a & (a - 1)) ? (uint32_t)a : 1u;
}
// File I/O helper threads.  Readers (compress_dir: open/pread/close, lstat) scale to ~16 threads; writers are fastest at ~4
// (the table is beside cut_writers, read_plan.h).  ZNIPPY_HOST_READERS / ZNIPPY_HOST_WRITERS override.
unsigned env_threads(const char *name, unsigned dflt) {
    unsigned hw = std::thread::hardware_concurrency();
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof set, &set) == 0) hw = (unsigned)CPU_COUNT(&set);
    const char *v = getenv(name);
    unsigned want = v && *v ? (unsigned)strtoul(v, nullptr, 10) : dflt;
    return std::max(1u, std::min(want, hw ? hw : 1u));
}
unsigned reader_threads() { return env_threads("ZNIPPY_HOST_READERS", 16); }
unsigned writer_threads() { return env_threads("ZNIPPY_HOST_WRITERS", 4); }

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
bool env_on(const char *name) { const char *v = getenv(name); return v && *v && *v != '0'; }
bool trace_on() { return env_on("ZNIPPY_HOST_TRACE"); }
const char MAGIC[8] = {'Z', 'N', 'P', 'Y', 'M', 'I', 'D', 'X'};  // index.rs:L245

// is_probably_compressed, index.rs:L470-484 — last extension, case-insensitive
bool should_skip_compression(const std::string &path) {
    static const char *exts[] = {"zip", "gz", "bz2", "xz", "lz", "lzma", "7z", "rar", "cab", "jar", "war", "ear",
                                 "zst", "sz", "lz4", "tgz", "txz", "tbz", "apk", "dmg", "deb", "rpm", "arrow",
                                 "mpeg", "mpg", "jpeg", "jpg", "gif", "bmp", "png", "crate", "znippy", "zdata",
                                 "parquet", "webp", "webm"};
    size_t slash = path.find_last_of('/');
    std::string name = slash == std::string::npos ? path : path.substr(slash + 1);
    size_t dot = name.find_last_of('.');
    if (dot == std::string::npos || dot == 0 || dot + 1 == name.size()) return false;  // ".gz" has no extension
    std::string ext = name.substr(dot + 1);
    for (auto &ch : ext) ch = (char)tolower((unsigned char)ch);
    for (const char *e : exts)
        if (ext == e) return true;
    return false;
}

std::string with_extension(const std::string &path, const char *ext) {  // Path::with_extension
    size_t slash = path.find_last_of('/');
    size_t start = slash == std::string::npos ? 0 : slash + 1;
    std::string name = path.substr(start);
    size_t dot = name.find_last_of('.');
    if (dot != std::string::npos && dot != 0) name = name.substr(0, dot);
    return path.substr(0, start) + name + "." + ext;
}

std::map<std::string, std::string> config_metadata() {  // index.rs:L73-85 over CONFIG (common_config.rs:L25-78)
    unsigned cores = std::thread::hardware_concurrency();
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof set, &set) == 0) cores = (unsigned)CPU_COUNT(&set);
    if (!cores) cores = 1;
    unsigned in_flight = (unsigned)std::ceil(cores * 0.90);
    long pages = sysconf(_SC_PHYS_PAGES), psz = sysconf(_SC_PAGE_SIZE);
    uint64_t mem = pages > 0 && psz > 0 ? (uint64_t)pages * (uint64_t)psz : 0;
    uint64_t max_chunks = std::min<uint64_t>(mem / (10ull * 1024 * 1024), 128);
    return {{"znippy_format_version", "3"},
            {"max_core_in_flight", std::to_string(in_flight)},
            {"max_core_in_compress", std::to_string(cores > in_flight ? cores - in_flight : 0)},
            {"max_mem_allowed", std::to_string(mem)},
            {"min_free_memory_ratio", "0"},
            {"file_split_block_size", std::to_string(10 * 1024 * 1024)},
            {"max_chunks", std::to_string(max_chunks)},
            {"compression_level", "19"},
            {"zstd_output_buffer_size", std::to_string(1024 * 1024)}};
}

aipc::Batch index_schema() {  // index.rs:L43-54
    aipc::Batch b;
    const char *names[8] = {"relative_path", "chunk_seq", "fdata_offset", "compressed", "uncompressed_size",
                            "blob_offset", "blob_size", "checksum"};
    const aipc::Kind kinds[8] = {aipc::Kind::Utf8, aipc::Kind::UInt32, aipc::Kind::UInt64, aipc::Kind::Bool,
                                 aipc::Kind::UInt64, aipc::Kind::UInt64, aipc::Kind::UInt64, aipc::Kind::FixedBin32};
    for (int i = 0; i < 8; i++) {
        aipc::Column c;
        c.name = names[i];
        c.kind = kinds[i];
        b.cols.push_back(c);
    }
    return b;
}

aipc::Batch manifest_schema() {  // index.rs:L279-288
    aipc::Batch b;
    const char *names[6] = {"pkg_type", "repo", "module_name", "index_offset", "index_len", "row_count"};
    const aipc::Kind kinds[6] = {aipc::Kind::Int8, aipc::Kind::Utf8, aipc::Kind::Utf8, aipc::Kind::UInt64,
                                 aipc::Kind::UInt64, aipc::Kind::UInt64};
    for (int i = 0; i < 6; i++) {
        aipc::Column c;
        c.name = names[i];
        c.kind = kinds[i];
        b.cols.push_back(c);
    }
    return b;
}

struct Manifest {
    int8_t pkg_type;
    std::string repo, module_name;
    uint64_t index_offset, index_len, row_count;
};

std::vector<uint8_t> manifest_bytes(const std::vector<Manifest> &m) {
    aipc::Batch b = manifest_schema();
    for (const auto &e : m) {
        b.cols[0].u8.push_back((uint8_t)e.pkg_type);
        b.cols[1].str.push_back(e.repo);
        b.cols[2].str.push_back(e.module_name);
        b.cols[3].u64.push_back(e.index_offset);
        b.cols[4].u64.push_back(e.index_len);
        b.cols[5].u64.push_back(e.row_count);
    }
    return aipc::write_stream({b}, manifest_schema(), {});
}

// ---- device buffer (grow-only) ----
struct DevBuf {
    uint8_t *p = nullptr;
    size_t cap = 0;
    bool reserve(size_t n) {
        if (n <= cap && p) return true;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        size_t want = std::max<size_t>(n + 64, 1 << 20);
        if (hipMalloc(&p, want) != hipSuccess) return false;
        cap = want;
        return true;
    }
    ~DevBuf() { if (p) (void)hipFree(p); }
};

// ---- page-locked host buffer (grow-only): DMA source/target, faulted in once and reused ----
struct PinBuf {
    uint8_t *p = nullptr;
    size_t cap = 0;
    bool reserve(size_t n) {
        if (n <= cap && p) return true;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
        size_t want = std::max<size_t>(n, 1 << 20);
        if (hipHostMalloc((void **)&p, want, hipHostMallocDefault) != hipSuccess) { p = nullptr; return false; }
        cap = want;
        return true;
    }
    ~PinBuf() { if (p) (void)hipHostFree(p); }
};

bool pread_all(int fd, void *dst, size_t n, uint64_t off) {
    uint8_t *d = (uint8_t *)dst;
    while (n) {
        ssize_t r = pread(fd, d, n, (off_t)off);
        if (r <= 0) return false;
        d += r; off += (uint64_t)r; n -= (size_t)r;
    }
    return true;
}
bool pwrite_all(int fd, const void *src, size_t n, uint64_t off) {
    const uint8_t *s = (const uint8_t *)src;
    while (n) {
        ssize_t r = pwrite(fd, s, n, (off_t)off);
        if (r <= 0) return false;
        s += r; off += (uint64_t)r; n -= (size_t)r;
    }
    return true;
}

void mkdirs(const std::string &dir) {
    if (dir.empty()) return;
    std::string cur;
    for (size_t i = 0; i < dir.size(); i++) {
        cur += dir[i];
        if (dir[i] == '/' || i + 1 == dir.size()) mkdir(cur.c_str(), 0755);
    }
}

using zn::IndexView;
using zn::RowTable;
static_assert(zn::RDP_E_CORRUPT == ZNIPPY_E_CORRUPT, "read_plan.h gives out ZNIPPY_E_CORRUPT");

}  // namespace

struct znippy_index {
    aipc::Batch rows = index_schema();
    std::vector<Manifest> manifest;
    std::map<std::string, std::string> metadata;
    uint64_t blob_end = 0, file_size = 0;
    size_t n() const { return rows.rows(); }
    IndexView view() const {  // the eight base columns by name (load_index_impl has put them in index_schema()'s order)
        const auto &c = rows.cols;
        IndexView v;
        v.path = c[0].str.data(); v.chunk_seq = c[1].u32.data(); v.fdata_offset = c[2].u64.data(); v.compressed = c[3].u8.data();
        v.usize = c[4].u64.data(); v.blob_offset = c[5].u64.data(); v.blob_size = c[6].u64.data(); v.checksum = c[7].u8.data();
        v.n = n(); v.file_size = file_size;
        return v;
    }
};

// A file is untrusted input: every length is checked against the file before anything is allocated or indexed,
// every read is checked, the manifest's columns are checked against the schema before they are indexed.
static int load_index_impl(const char *path, znippy_index *ix) {
    int fd = open(path, O_RDONLY);
    if (fd < 0) return fail(ZNIPPY_E_INVAL, std::string("cannot open ") + path);
    struct stat st;
    if (fstat(fd, &st) != 0) { close(fd); return fail(ZNIPPY_E_INVAL, std::string("cannot stat ") + path); }
    ix->file_size = (uint64_t)st.st_size;
    if (ix->file_size < 16) { close(fd); return fail(ZNIPPY_E_CORRUPT, "file too small to be a v0.7 znippy archive"); }
    uint8_t tail[16];
    if (!pread_all(fd, tail, 16, ix->file_size - 16)) { close(fd); return fail(ZNIPPY_E_CORRUPT, "cannot read the footer"); }
    uint64_t moff;
    if (!znippy_interpret_footer(tail, 16, &moff)) {
        close(fd);
        return fail(ZNIPPY_E_UNSUPPORTED, "v0.6 archives are not supported; re-compress with v0.7");  // index.rs:L387-389
    }
    const uint64_t mend = ix->file_size - 16;
    if (moff > mend) { close(fd); return fail(ZNIPPY_E_CORRUPT, "corrupt v0.7 manifest_offset"); }
    std::vector<uint8_t> mb(mend - moff);
    if (!mb.empty() && !pread_all(fd, mb.data(), mb.size(), moff)) { close(fd); return fail(ZNIPPY_E_CORRUPT, "cannot read the manifest"); }
    aipc::Batch m;
    std::string err;
    if (!aipc::read_stream(mb.data(), mb.size(), &m, nullptr, &err) || m.cols.size() != 6) {
        close(fd);
        return fail(ZNIPPY_E_CORRUPT, "manifest: " + err);
    }
    {  // the six manifest columns, by kind and with equal row counts (index.rs:L279-288)
        const aipc::Batch want = manifest_schema();
        const size_t nr = m.cols[0].rows();
        for (size_t c = 0; c < 6; c++)
            if (m.cols[c].kind != want.cols[c].kind || m.cols[c].rows() != nr) {
                close(fd);
                return fail(ZNIPPY_E_CORRUPT, "manifest: column " + want.cols[c].name + " has the wrong type or length");
            }
    }
    ix->blob_end = moff;
    for (size_t i = 0; i < m.rows(); i++) {
        Manifest e{(int8_t)m.cols[0].u8[i], m.cols[1].str[i], m.cols[2].str[i], m.cols[3].u64[i], m.cols[4].u64[i],
                   m.cols[5].u64[i]};
        ix->blob_end = std::min(ix->blob_end, e.index_offset);
        ix->manifest.push_back(e);
    }
    ix->rows.cols.clear();
    bool first = true;
    for (const auto &e : ix->manifest) {
        if (e.index_offset > ix->file_size || e.index_len > ix->file_size - e.index_offset) { close(fd); return fail(ZNIPPY_E_CORRUPT, "sub-index out of range"); }
        std::vector<uint8_t> sb(e.index_len);
        if (!sb.empty() && !pread_all(fd, sb.data(), sb.size(), e.index_offset)) { close(fd); return fail(ZNIPPY_E_CORRUPT, "cannot read a sub-index"); }
        if (!aipc::read_stream(sb.data(), sb.size(), &ix->rows, first ? &ix->metadata : nullptr, &err)) {
            close(fd);
            return fail(ZNIPPY_E_CORRUPT, "sub-index: " + err);
        }
        first = false;
    }
    close(fd);
    if (ix->rows.cols.empty()) ix->rows = index_schema();
    // locate the 8 base columns by name (module columns may follow them)
    const aipc::Batch want = index_schema();
    aipc::Batch ordered;
    for (const auto &wc : want.cols) {
        bool found = false;
        for (auto &c : ix->rows.cols)
            if (c.name == wc.name && c.kind == wc.kind) { ordered.cols.push_back(std::move(c)); found = true; break; }
        if (!found) return fail(ZNIPPY_E_CORRUPT, "index is missing column " + wc.name);
    }
    ix->rows = std::move(ordered);
    const size_t nr = ix->rows.cols[0].rows();
    for (const auto &c : ix->rows.cols)
        if (c.rows() != nr) return fail(ZNIPPY_E_CORRUPT, "index column " + c.name + " has the wrong length");
    return ZNIPPY_OK;
}

// No C++ exception crosses the C ABI: allocation failures and anything a parser throws become status codes.
template <class F>
static int guarded(F &&f) {
    try {
        return f();
    } catch (const std::bad_alloc &) {
        return fail(ZNIPPY_E_NOMEM, "out of host memory");
    } catch (const std::exception &e) {
        return fail(ZNIPPY_E_CORRUPT, std::string("malformed input: ") + e.what());
    } catch (...) {
        return fail(ZNIPPY_E_CORRUPT, "malformed input");
    }
}

static int load_index(const char *path, znippy_index *ix) {
    return guarded([&] { return load_index_impl(path, ix); });
}

namespace {

// ---------------------------------------------------------------------------------------------------
// Write side.  Rounds are laid into page-locked staging slots in reservation order; a device thread takes
// full slots (H2D -> encode+hash kernels -> D2H of the packed blobs -> pwrite) while the producer fills the
// next one.  Stands for the reader -> barrel -> writer channel chain of stream_packer.rs:L146-284 and the
// Magazine of slot_packer.rs:L222-330: the channels carry slots instead of Rounds, the barrels are kernels.
struct RoundRec {
    uint32_t file_index, chunk_seq;
    uint64_t fdata_offset, len, pos;  // pos = byte position in the slot
    bool skip;
    uint8_t pass;                     // compress_dir: 0 = big pass, 1 = small pass
};

struct RowMeta {  // BlobMeta + ChunkMeta, meta.rs:L4-21
    uint32_t file_index, chunk_seq;
    uint64_t fdata_offset, usize, blob_offset, blob_size;
    bool compressed;
    uint8_t pass;
    uint8_t checksum[32];
    uint64_t tree_at;  // ZNIPPY_HOST_BLOCK_TREE: the row's block tree entries in Packer::tree (byte position), tree_n of them
    uint32_t tree_n;
};

struct StageSlot {
    PinBuf buf;
    size_t used = 0;
    std::vector<RoundRec> rounds;
    std::atomic<int> pending{0};  // asynchronous reads still landing in this slot
};

class Packer {
public:
    Packer(int fd, int device, uint64_t max_round)
        : emit_tree(env_on("ZNIPPY_HOST_BLOCK_TREE")), fd_(fd), device_(device), slot_cap_(std::max(stage_bytes(), max_round)), align_(blob_align()) {}
    ~Packer() {
        if (thread_.joinable()) { push_full(nullptr); thread_.join(); }
        if (ctx_) znippy_ctx_destroy(ctx_);
    }
    int start() {
        hipError_t e = hipSetDevice(device_);
        if (e != hipSuccess) return fail(ZNIPPY_E_HIP, std::string("hipSetDevice failed: ") + hipGetErrorString(e));
        int rc = znippy_ctx_create(device_, nullptr, &ctx_);
        if (rc) return fail(rc, "znippy_ctx_create failed: no usable GPU (the codec/hash path has no CPU fallback)");
        for (auto &s : slots_) free_.push_back(&s);
        thread_ = std::thread([this] { run(); });
        return ZNIPPY_OK;
    }
    // Reserve r.len bytes for the next round.  async = the bytes arrive later (reader threads call landed()).
    uint8_t *reserve(RoundRec r, bool async, StageSlot **slot_out = nullptr) {
        if (!cur_ || cur_->used + r.len > cur_->buf.cap || cur_->rounds.size() >= MAX_SLOT_ROUNDS) {
            if (cur_) push_full(cur_);
            cur_ = pop_free();
            if (!cur_->buf.reserve(slot_cap_)) { set_error(ZNIPPY_E_NOMEM, "page-locked staging allocation failed"); return nullptr; }
        }
        r.pos = cur_->used;
        cur_->rounds.push_back(r);
        cur_->used += r.len;
        if (async && r.len) cur_->pending.fetch_add(1, std::memory_order_relaxed);
        if (slot_out) *slot_out = cur_;
        return cur_->buf.p + r.pos;
    }
    // True when the next reserve(len) has to hand the current slot over (and may wait for a free one).
    bool would_switch(uint64_t len) const { return !cur_ || cur_->used + len > cur_->buf.cap || cur_->rounds.size() >= MAX_SLOT_ROUNDS; }
    void landed(StageSlot *s) {
        if (s->pending.fetch_sub(1, std::memory_order_acq_rel) == 1) {  // lock so that the wake cannot slip past the waiter's check
            std::lock_guard<std::mutex> g(mu_);
            cv_.notify_all();
        }
    }
    void set_error(int rc, const std::string &msg) {
        std::lock_guard<std::mutex> g(mu_);
        if (!rc_) { rc_ = rc; err_ = msg; }
    }
    int error() { std::lock_guard<std::mutex> g(mu_); return rc_; }
    // Flush, wait for the device thread, return the pipeline status (message via fail()).
    int finish() {
        if (cur_) { push_full(cur_); cur_ = nullptr; }
        push_full(nullptr);
        thread_.join();
        if (trace_on())
            fprintf(stderr, "[host] write: slots %d  wait %.1f ms  h2d %.1f ms  kernels %.1f ms  d2h %.1f ms  pwrite %.1f ms\n", n_slots_,
                    t_wait_ * 1e3, t_h2d_ * 1e3, t_kern_ * 1e3, t_d2h_ * 1e3, t_write_ * 1e3);
        return rc_ ? fail(rc_, "compress pipeline failed: " + err_) : ZNIPPY_OK;
    }
    std::vector<RowMeta> rows;
    uint64_t out_cursor = 0;  // blob region starts at 0 (stream_packer.rs:L134)
    const bool emit_tree;       // ZNIPPY_HOST_BLOCK_TREE, read when the pipeline starts: every slot's rounds table emits its block tree
    std::vector<uint8_t> tree;  // ... and the slots' trees are kept here, found by row through RowMeta::tree_at

private:
    void push_full(StageSlot *s) {
        std::lock_guard<std::mutex> g(mu_);
        full_.push_back(s);
        cv_.notify_all();
    }
    StageSlot *pop_free() {
        std::unique_lock<std::mutex> g(mu_);
        cv_.wait(g, [this] { return !free_.empty(); });
        StageSlot *s = free_.front();
        free_.pop_front();
        return s;
    }
    void run() {
        (void)hipSetDevice(device_);
        for (;;) {
            StageSlot *s;
            const double t0 = now_s();
            {
                std::unique_lock<std::mutex> g(mu_);
                cv_.wait(g, [this] { return !full_.empty(); });
                s = full_.front();
                full_.pop_front();
                if (s) cv_.wait(g, [s] { return s->pending.load(std::memory_order_acquire) == 0; });
            }
            t_wait_ += now_s() - t0;
            if (!s) return;
            if (!error()) {
                std::string msg;
                int rc = process(*s, &msg);
                if (rc) set_error(rc, msg);
            }
            s->used = 0;
            s->rounds.clear();
            std::lock_guard<std::mutex> g(mu_);
            free_.push_back(s);
            cv_.notify_all();
        }
    }
    int process(StageSlot &s, std::string *msg) {
        const size_t nb = s.rounds.size();
        if (!nb) return ZNIPPY_OK;
        n_slots_++;
        std::vector<uint64_t> off(nb), len(nb), boff(nb), bsz(nb);
        std::vector<uint8_t> skip(nb), comp(nb), ck(32 * nb);
        for (size_t k = 0; k < nb; k++) { off[k] = s.rounds[k].pos; len[k] = s.rounds[k].len; skip[k] = s.rounds[k].skip; }
        double t = now_s();
        if (!d_src_.reserve(s.buf.cap + 64)) { *msg = "device staging allocation failed"; return ZNIPPY_E_NOMEM; }
        if (s.used && hipMemcpy(d_src_.p, s.buf.p, s.used, hipMemcpyHostToDevice) != hipSuccess) { *msg = "H2D failed"; return ZNIPPY_E_HIP; }
        t_h2d_ += now_s() - t; t = now_s();
        znippy_rounds *rt = nullptr;
        uint64_t blob_bytes = 0;
        int rc = znippy_rounds_create(ctx_, off.data(), len.data(), skip.data(), nb, &rt);
        if (!rc && align_ > 1) rc = znippy_rounds_set_blob_align(rt, align_);
        if (!rc && emit_tree) rc = znippy_rounds_emit_block_tree(rt, 1);
        if (!rc && !d_blob_.reserve(znippy_rounds_blob_bound(rt) + 64)) rc = ZNIPPY_E_NOMEM;  // (the bound follows the alignment)
        if (!rc) rc = znippy_encode_hash_rounds(ctx_, rt, d_src_.p, d_blob_.p, d_blob_.cap, boff.data(), bsz.data(), ck.data(), comp.data(), &blob_bytes);
        std::vector<uint64_t> tfirst(nb + 1, 0);
        const size_t tree_base = tree.size();
        if (!rc && emit_tree) {  // the slot's tree arrived with its results: kept by row until the metadata layer is written
            uint64_t ne = 0;
            rc = znippy_rounds_block_tree_layout(ctx_, rt, &ne, tfirst.data());
            if (!rc) {
                tree.resize(tree_base + 32 * (size_t)ne);
                rc = znippy_rounds_block_tree(ctx_, rt, 0, ne ? tree.data() + tree_base : nullptr);
            }
        }
        if (rt) znippy_rounds_destroy(rt);
        if (rc) { *msg = znippy_last_error(ctx_); return rc; }
        t_kern_ += now_s() - t; t = now_s();
        if (!blob_pin_.reserve(blob_bytes)) { *msg = "page-locked blob allocation failed"; return ZNIPPY_E_NOMEM; }
        if (blob_bytes && hipMemcpy(blob_pin_.p, d_blob_.p, blob_bytes, hipMemcpyDeviceToHost) != hipSuccess) { *msg = "D2H failed"; return ZNIPPY_E_HIP; }
        t_d2h_ += now_s() - t; t = now_s();
        out_cursor = (out_cursor + align_ - 1) & ~(uint64_t)(align_ - 1);  // aligned blob offsets: the hole in front of the slot reads as zeros
        if (!pwrite_all(fd_, blob_pin_.p, blob_bytes, out_cursor)) { *msg = "archive write failed"; return ZNIPPY_E_INVAL; }  // the writer, L255-284
        t_write_ += now_s() - t;
        for (size_t k = 0; k < nb; k++) {
            const RoundRec &r = s.rounds[k];
            RowMeta m{r.file_index, r.chunk_seq, r.fdata_offset, r.len, out_cursor + boff[k], bsz[k], comp[k] != 0, r.pass, {0},
                      tree_base + 32 * (size_t)tfirst[k], (uint32_t)(tfirst[k + 1] - tfirst[k])};
            std::memcpy(m.checksum, &ck[32 * k], 32);
            rows.push_back(m);
        }
        out_cursor += blob_bytes;
        return ZNIPPY_OK;
    }

    int fd_, device_;
    uint64_t slot_cap_;
    uint32_t align_;
    znippy_ctx *ctx_ = nullptr;
    StageSlot slots_[N_STAGE];
    StageSlot *cur_ = nullptr;
    std::deque<StageSlot *> free_, full_;
    std::mutex mu_;
    std::condition_variable cv_;
    std::thread thread_;
    int rc_ = 0;
    std::string err_;
    DevBuf d_src_, d_blob_;
    PinBuf blob_pin_;
    int n_slots_ = 0;
    double t_wait_ = 0, t_h2d_ = 0, t_kern_ = 0, t_d2h_ = 0, t_write_ = 0;
};

// The metadata layer: one Arrow-IPC sub-index stream per group, then manifest + footer (ArrowIpcSink,
// meta_sink.rs:L71-118).  Returns total_bytes_out.
struct SubIndex {
    int8_t pkg_type;
    std::string repo;
    std::vector<std::vector<size_t>> batches;  // row numbers per record batch
};

template <class PathOf>
uint64_t write_metadata(int fd, uint64_t blob_end, const std::vector<RowMeta> &rows, PathOf path_of, const std::vector<SubIndex> &subs) {
    const auto meta = config_metadata();
    uint64_t cursor = blob_end;
    std::vector<Manifest> manifest;
    for (const auto &g : subs) {
        std::vector<aipc::Batch> bs;
        uint64_t n_rows = 0;
        for (const auto &ids : g.batches) {
            aipc::Batch b = index_schema();
            for (size_t k : ids) {
                const RowMeta &m = rows[k];
                b.cols[0].str.push_back(path_of(m.file_index));
                b.cols[1].u32.push_back(m.chunk_seq);
                b.cols[2].u64.push_back(m.fdata_offset);
                b.cols[3].u8.push_back(m.compressed);
                b.cols[4].u64.push_back(m.usize);
                b.cols[5].u64.push_back(m.blob_offset);
                b.cols[6].u64.push_back(m.blob_size);
                b.cols[7].u8.insert(b.cols[7].u8.end(), m.checksum, m.checksum + 32);
            }
            n_rows += ids.size();
            bs.push_back(std::move(b));
        }
        std::vector<uint8_t> sub = aipc::write_stream(bs, index_schema(), meta);
        pwrite_all(fd, sub.data(), sub.size(), cursor);  // push_subindex, meta_sink.rs:L71-101
        manifest.push_back({g.pkg_type, g.repo, "", cursor, sub.size(), n_rows});
        cursor += sub.size();
    }
    const uint64_t manifest_offset = cursor;  // finish, meta_sink.rs:L103-118
    std::vector<uint8_t> mb = manifest_bytes(manifest);
    pwrite_all(fd, mb.data(), mb.size(), cursor);
    cursor += mb.size();
    pwrite_all(fd, MAGIC, 8, cursor);
    pwrite_all(fd, &manifest_offset, 8, cursor + 8);
    fsync(fd);
    return cursor + 16;
}

// The block tree sidecar `<archive path>.b3t` (znippy_host.h): header + the rows' entries in the order the index numbers the rows —
// sub-index by sub-index, batch by batch, as write_metadata lays them down.
using zn::B3T_BLOCK_LOG;
using zn::B3T_HEADER;
using zn::B3T_MAGIC;

bool write_sidecar(const std::string &archive_path, const std::vector<RowMeta> &rows, const std::vector<uint8_t> &tree, const std::vector<SubIndex> &subs) {
    std::vector<uint8_t> out(B3T_HEADER, 0);
    uint64_t n_rows = 0;
    for (const auto &g : subs)
        for (const auto &ids : g.batches)
            for (size_t k : ids) {
                const RowMeta &m = rows[k];
                out.insert(out.end(), tree.begin() + m.tree_at, tree.begin() + m.tree_at + 32 * (size_t)m.tree_n);
                n_rows++;
            }
    const uint64_t n_entries = (out.size() - B3T_HEADER) / 32;
    const uint32_t log = B3T_BLOCK_LOG;
    std::memcpy(out.data(), B3T_MAGIC, 8);
    std::memcpy(out.data() + 8, &log, 4);
    std::memcpy(out.data() + 16, &n_rows, 8);
    std::memcpy(out.data() + 24, &n_entries, 8);
    const std::string path = archive_path + ".b3t";
    const int fd = open(path.c_str(), O_CREAT | O_TRUNC | O_WRONLY, 0644);
    if (fd < 0) return false;
    const bool ok = pwrite_all(fd, out.data(), out.size(), 0);
    close(fd);
    return ok;
}

struct FileMeta {
    std::string path;
    int pkg_type;  // < 0 = None
    bool has_repo;
    std::string repo;
};

}  // namespace

struct znippy_stream {
    std::string out_path;
    bool no_skip = false;
    int fd = -1;
    std::unique_ptr<Packer> packer;
    std::vector<FileMeta> files;
    uint64_t uf = 0, ub = 0, cf = 0, cb = 0;
    double t_open = 0, t_send = 0;
    ~znippy_stream() {
        packer.reset();
        if (fd >= 0) close(fd);
    }
};

extern "C" {

const char *znippy_host_last_error(void) { return g_err.c_str(); }

int znippy_interpret_footer(const uint8_t *tail, size_t n, uint64_t *offset) {
    if (n < 8) return 0;
    std::memcpy(offset, tail + n - 8, 8);
    return n >= 16 && std::memcmp(tail + n - 16, MAGIC, 8) == 0;
}

size_t znippy_write_manifest_bytes(const znippy_manifest_entry *entries, size_t n, uint8_t *dst, size_t cap) {
    std::vector<Manifest> m;
    for (size_t i = 0; i < n; i++)
        m.push_back({entries[i].pkg_type, entries[i].repo ? entries[i].repo : "", entries[i].module_name ? entries[i].module_name : "",
                     entries[i].index_offset, entries[i].index_len, entries[i].row_count});
    std::vector<uint8_t> b = manifest_bytes(m);
    if (dst && cap) std::memcpy(dst, b.data(), std::min(cap, b.size()));
    return b.size();
}

// ---- write side: compress_stream --------------------------------------------------------------
static int znippy_compress_stream_impl(const char *output, int no_skip, int device, znippy_stream **out) {
    if (!output || !out) return fail(ZNIPPY_E_INVAL, "null argument");
    std::unique_ptr<znippy_stream> s(new znippy_stream());
    s->t_open = now_s();
    s->out_path = with_extension(output, "znippy");  // stream_packer.rs:L132
    s->no_skip = no_skip != 0;
    s->fd = open(s->out_path.c_str(), O_CREAT | O_TRUNC | O_RDWR, 0644);
    if (s->fd < 0) return fail(ZNIPPY_E_INVAL, "cannot create " + s->out_path);
    s->packer.reset(new Packer(s->fd, device, SLICE_SIZE));
    int rc = s->packer->start();
    if (rc) return rc;
    *out = s.release();
    return ZNIPPY_OK;
}

// The reader's chunking (stream_packer.rs:L146-206) runs on the caller's thread: each entry is cut into
// Rounds and copied once, straight into page-locked staging.
static int znippy_stream_send_impl(znippy_stream *s, const char *relative_path, const void *data, size_t len, int pkg_type,
                       const char *repo) {
    if (!s || !relative_path || (len && !data)) return fail(ZNIPPY_E_INVAL, "null argument");
    const double t0 = now_s();
    const uint32_t fi = (uint32_t)s->files.size();
    s->files.push_back({relative_path, pkg_type, repo != nullptr, repo ? repo : ""});
    const bool skip = !s->no_skip && should_skip_compression(s->files.back().path);
    if (skip) { s->uf++; s->ub += len; } else { s->cf++; s->cb += len; }
    if (len == 0) {  // L169-183: one zero-length row
        if (!s->packer->reserve({fi, 0, 0, 0, 0, skip, 0}, false)) return fail(ZNIPPY_E_NOMEM, "staging allocation failed");
    } else {
        const bool small = len <= SLICE_SIZE;
        uint64_t off = 0;
        uint32_t seq = 0;
        while (off < len) {
            const uint64_t n = small ? len : std::min<uint64_t>(SLICE_SIZE, len - off);
            uint8_t *dst = s->packer->reserve({fi, seq, off, n, 0, skip, 0}, false);
            if (!dst) return fail(ZNIPPY_E_NOMEM, "staging allocation failed");
            std::memcpy(dst, (const uint8_t *)data + off, n);
            off += n;
            seq++;
        }
    }
    s->t_send += now_s() - t0;
    return ZNIPPY_OK;
}

static int znippy_stream_send_packed_impl(znippy_stream *s, uint64_t n, const char *paths, const uint64_t *path_off, const void *data,
                                          const uint64_t *data_off, const int32_t *pkg_type, const char *repo) {
    if (!s || (n && (!paths || !path_off || !data_off))) return fail(ZNIPPY_E_INVAL, "null argument");
    std::string path;
    for (uint64_t i = 0; i < n; i++) {
        if (path_off[i + 1] < path_off[i] || data_off[i + 1] < data_off[i]) return fail(ZNIPPY_E_INVAL, "offsets must not decrease");
        path.assign(paths + path_off[i], paths + path_off[i + 1]);
        const uint64_t len = data_off[i + 1] - data_off[i];
        if (len && !data) return fail(ZNIPPY_E_INVAL, "null data");
        const int rc = znippy_stream_send_impl(s, path.c_str(), len ? (const uint8_t *)data + data_off[i] : nullptr, (size_t)len,
                                               pkg_type ? (int)pkg_type[i] : -1, repo);
        if (rc) return rc;
    }
    return ZNIPPY_OK;
}

static int znippy_stream_finish_impl(znippy_stream *sp, znippy_compression_report *report) {
    if (!sp) return fail(ZNIPPY_E_INVAL, "null stream");
    std::unique_ptr<znippy_stream> s(sp);
    const double t0 = now_s();
    int rc = s->packer->finish();
    if (rc) return rc;
    const double t1 = now_s();
    std::vector<RowMeta> &rows = s->packer->rows;
    // finalizer (L293-346): rows sorted by (file_index, chunk_seq), grouped by (pkg_type, repo) in BTreeMap order
    std::stable_sort(rows.begin(), rows.end(), [](const RowMeta &a, const RowMeta &b) {
        return a.file_index != b.file_index ? a.file_index < b.file_index : a.chunk_seq < b.chunk_seq;
    });
    std::map<std::pair<int8_t, std::string>, std::vector<size_t>> groups;
    for (size_t k = 0; k < rows.size(); k++) {
        const FileMeta &e = s->files[rows[k].file_index];
        groups[{(int8_t)(e.pkg_type < 0 ? 0 : e.pkg_type), e.has_repo ? e.repo : std::string()}].push_back(k);
    }
    std::vector<SubIndex> subs;
    for (auto &g : groups) subs.push_back({g.first.first, g.first.second, {std::move(g.second)}});
    const uint64_t total_bytes_out =
        write_metadata(s->fd, s->packer->out_cursor, rows, [&](uint32_t fi) -> const std::string & { return s->files[fi].path; }, subs);
    if (s->packer->emit_tree && !write_sidecar(s->out_path, rows, s->packer->tree, subs)) return fail(ZNIPPY_E_INVAL, "cannot write " + s->out_path + ".b3t");
    if (trace_on())
        fprintf(stderr, "[host] compress_stream: open->finish %.1f ms (send calls %.1f ms)  drain %.1f ms  metadata %.1f ms\n",
                (t0 - s->t_open) * 1e3, s->t_send * 1e3, (t1 - t0) * 1e3, (now_s() - t1) * 1e3);
    if (report) {
        *report = znippy_compression_report{s->uf + s->cf, s->cf, s->uf, 0, s->cb + s->ub, total_bytes_out, s->cb, s->ub, (uint64_t)rows.size(),
                                            (s->cb > 0 && total_bytes_out > s->ub) ? (float)s->cb / (float)(total_bytes_out - s->ub) * 100.0f : 0.0f};
    }
    return ZNIPPY_OK;
}

// ---- write side: compress_dir (slot_packer.rs:L55-209) ------------------------------------------
}  // extern "C"

namespace {

// WalkDir order (L63-78): a directory's files, then its sub-directories, both in name order; only regular
// files are ingested, every directory (the root too) is counted.
void walk_dir(const std::string &dir, std::vector<std::string> *files, uint64_t *n_dirs) {
    DIR *d = opendir(dir.c_str());
    if (!d) return;
    (*n_dirs)++;
    std::vector<std::string> fs, ds;
    while (struct dirent *e = readdir(d)) {
        const std::string name = e->d_name;
        if (name == "." || name == "..") continue;
        if (e->d_type == DT_DIR) { ds.push_back(name); continue; }
        if (e->d_type == DT_REG) { fs.push_back(name); continue; }
        if (e->d_type != DT_UNKNOWN) continue;
        struct stat st;  // a file system that does not report entry types
        if (lstat((dir + "/" + name).c_str(), &st) != 0) continue;
        if (S_ISDIR(st.st_mode)) ds.push_back(name);
        else if (S_ISREG(st.st_mode)) fs.push_back(name);
    }
    closedir(d);
    std::sort(fs.begin(), fs.end());
    std::sort(ds.begin(), ds.end());
    for (const auto &f : fs) files->push_back(dir + "/" + f);
    for (const auto &sub : ds) walk_dir(dir + "/" + sub, files, n_dirs);
}

// file sizes, a few threads at a time (100k lstat calls are the larger half of a serial walk)
void stat_sizes(const std::vector<std::string> &files, std::vector<uint64_t> *sizes) {
    sizes->assign(files.size(), 0);
    const unsigned nt = std::max(1u, std::min<unsigned>(reader_threads(), (unsigned)(files.size() / 1024 + 1)));
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; t++)
        th.emplace_back([&, t] {
            for (size_t i = t; i < files.size(); i += nt) {
                struct stat st;
                if (lstat(files[i].c_str(), &st) == 0) (*sizes)[i] = (uint64_t)st.st_size;
            }
        });
    for (auto &x : th) x.join();
}

struct ReadTask {
    uint32_t file_index;
    uint64_t off, len;
    uint8_t *dst;
    StageSlot *slot;
};

// File readers feeding the staging slots (the io_uring reader's job, slot_packer.rs:L236-330, as plain
// positional reads on a few threads — the device path downstream is what this library is about).
class ReaderPool {
public:
    ReaderPool(Packer *pk, const std::vector<std::string> *files, unsigned n) : pk_(pk), files_(files) {
        for (unsigned i = 0; i < n; i++) th_.emplace_back([this] { run(); });
    }
    // Tasks are handed over in batches (one lock + wake per batch, not per file); flush() before anything that
    // may wait for a slot to drain.
    void push(const ReadTask &t) {
        batch_.push_back(t);
        if (batch_.size() >= 256) flush();
    }
    void flush() {
        if (batch_.empty()) return;
        std::lock_guard<std::mutex> g(mu_);
        q_.insert(q_.end(), batch_.begin(), batch_.end());
        batch_.clear();
        cv_.notify_all();
    }
    void join() {
        flush();
        {
            std::lock_guard<std::mutex> g(mu_);
            done_ = true;
            cv_.notify_all();
        }
        for (auto &t : th_) t.join();
        th_.clear();
    }
    ~ReaderPool() { if (!th_.empty()) join(); }

private:
    void run() {
        int fd = -1;
        uint32_t cur = UINT32_MAX;
        for (;;) {
            ReadTask ts[16];
            int nt = 0;
            {
                std::unique_lock<std::mutex> g(mu_);
                cv_.wait(g, [this] { return done_ || !q_.empty(); });
                if (q_.empty()) break;
                while (nt < 16 && !q_.empty()) { ts[nt++] = q_.front(); q_.pop_front(); }
            }
            for (int i = 0; i < nt; i++) {
                const ReadTask &t = ts[i];
                if (t.file_index != cur) {
                    if (fd >= 0) close(fd);
                    fd = open((*files_)[t.file_index].c_str(), O_RDONLY);
                    cur = t.file_index;
                }
                if (fd < 0 || !pread_all(fd, t.dst, t.len, t.off)) pk_->set_error(ZNIPPY_E_INVAL, "failed to read " + (*files_)[t.file_index]);
                pk_->landed(t.slot);
            }
        }
        if (fd >= 0) close(fd);
    }
    Packer *pk_;
    const std::vector<std::string> *files_;
    std::vector<std::thread> th_;
    std::deque<ReadTask> q_;
    std::vector<ReadTask> batch_;
    std::mutex mu_;
    std::condition_variable cv_;
    bool done_ = false;
};

}  // namespace

extern "C" {

static int znippy_compress_dir_impl(const char *input_dir, const char *output, int no_skip, const char *repo, int device,
                        znippy_compression_report *report) {
    if (!input_dir || !output) return fail(ZNIPPY_E_INVAL, "null argument");
    const double t_begin = now_s();
    std::string root = input_dir;
    while (root.size() > 1 && root.back() == '/') root.pop_back();
    std::vector<std::string> files;
    std::vector<uint64_t> sizes;
    uint64_t total_dirs = 0;
    walk_dir(root, &files, &total_dirs);
    stat_sizes(files, &sizes);
    const double t_walk = now_s();
    unsigned cores = std::thread::hardware_concurrency();
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof set, &set) == 0) cores = (unsigned)CPU_COUNT(&set);
    const uint64_t num_workers = std::max<uint64_t>((uint64_t)std::ceil(std::max(cores, 1u) * 0.90), 1);  // CONFIG.max_core_in_flight
    const uint64_t slice_size = SLOT_SIZE / num_workers;  // L89
    const std::string out_path = with_extension(output, "znippy");
    int fd = open(out_path.c_str(), O_CREAT | O_TRUNC | O_RDWR, 0644);
    if (fd < 0) return fail(ZNIPPY_E_INVAL, "cannot create " + out_path);
    uint64_t uf = 0, ub = 0, cf = 0, cb = 0;
    std::vector<RowMeta> rows;
    std::vector<uint8_t> tree;
    bool emit_tree = false;
    uint64_t blob_bytes = 0;
    {
        Packer pk(fd, device, std::max<uint64_t>(slice_size, 1));
        int rc = pk.start();
        if (rc) { close(fd); return rc; }
        ReaderPool readers(&pk, &files, reader_threads());
        bool ok = true;
        for (int pass = 0; pass < 2 && ok; pass++) {  // partition L92-101: pass 0 = big (or empty) files, pass 1 = small
            for (uint32_t i = 0; i < files.size() && ok; i++) {
                const uint64_t size = sizes[i];
                const bool big = size > slice_size || size == 0;
                if (big != (pass == 0)) continue;
                const bool skip = !no_skip && should_skip_compression(files[i]);
                if (skip) { uf++; ub += size; } else { cf++; cb += size; }
                uint64_t off = 0;
                uint32_t seq = 0;
                do {  // big: slice_size rounds with fdata_offset/chunk_seq (L265-280); small: one round (L499)
                    const uint64_t n = std::min(slice_size, size - off);
                    StageSlot *slot = nullptr;
                    if (pk.would_switch(n)) readers.flush();
                    uint8_t *dst = pk.reserve({i, seq, off, n, 0, skip, (uint8_t)pass}, true, &slot);
                    if (!dst) { ok = false; break; }
                    if (n) readers.push({i, off, n, dst, slot});
                    off += n;
                    seq++;
                } while (off < size);
            }
        }
        readers.join();
        rc = pk.finish();
        if (rc) { close(fd); return rc; }
        rows = std::move(pk.rows);
        tree = std::move(pk.tree);
        emit_tree = pk.emit_tree;
        blob_bytes = pk.out_cursor;
    }
    const double t_pack = now_s();
    // one sub-index, one record batch per non-empty pass, rows in round order (L141-189)
    SubIndex sub{0, repo ? repo : "", {}};
    for (uint8_t pass = 0; pass < 2; pass++) {
        std::vector<size_t> ids;
        for (size_t k = 0; k < rows.size(); k++)
            if (rows[k].pass == pass) ids.push_back(k);
        if (!ids.empty()) sub.batches.push_back(std::move(ids));
    }
    std::vector<std::string> rel(files.size());
    for (size_t i = 0; i < files.size(); i++) rel[i] = files[i].compare(0, root.size() + 1, root + "/") == 0 ? files[i].substr(root.size() + 1) : files[i];
    const uint64_t total_bytes_out = write_metadata(fd, blob_bytes, rows, [&](uint32_t fi) -> const std::string & { return rel[fi]; }, {sub});
    close(fd);
    if (emit_tree && !write_sidecar(out_path, rows, tree, {sub})) return fail(ZNIPPY_E_INVAL, "cannot write " + out_path + ".b3t");
    if (trace_on())
        fprintf(stderr, "[host] compress_dir: walk %.1f ms  pack %.1f ms  metadata %.1f ms\n", (t_walk - t_begin) * 1e3, (t_pack - t_walk) * 1e3,
                (now_s() - t_pack) * 1e3);
    if (report) {
        *report = znippy_compression_report{(uint64_t)files.size(), cf, uf, total_dirs, cb + ub, total_bytes_out, cb, ub, (uint64_t)rows.size(),
                                            ub > 0 ? (float)cb / (float)std::max<uint64_t>(blob_bytes, 1) * 100.0f : 0.0f};
    }
    return ZNIPPY_OK;
}

// ---- read side --------------------------------------------------------------------------------
}  // extern "C"

namespace {

struct DecodedRange {
    std::vector<uint64_t> out_off;  // position of each row's bytes in the decoded region
    std::vector<uint64_t> len;      // bytes of each row: uncompressed_size, or blob_size for a stored row (decompress.rs:L160-166)
    uint64_t total = 0;
    std::vector<int32_t> status;
    znippy_verify_counters cnt{};
    std::vector<uint64_t> corrupt;  // absolute row numbers
};

struct ReadBufs {
    DevBuf d_blobs, d_out;
    PinBuf blob_pin;
    double t_read = 0, t_h2d = 0, t_kern = 0;
};

bool read_into_slab(int fd, uint8_t *slab, const std::vector<zn::SlabRead> &reads) {
    for (const zn::SlabRead &r : reads)
        if (!pread_all(fd, slab + r.at, r.len, r.fpos)) return false;
    return true;
}

// A private device table of t's rows over a blob region of blob_cap bytes (~0: not declared): a row pointing outside what was
// read is an error code, not a device fault.
int create_rows(znippy_ctx *ctx, const RowTable &t, const uint64_t *out_off, uint64_t blob_cap, znippy_rows **rt) {
    const int rc = znippy_rows_create(ctx, t.bo.data(), t.bs.data(), t.bitmap.data(), t.us.data(), out_off, t.ck.empty() ? nullptr : t.ck.data(), 0, t.n(), rt);
    if (rc) return fail(rc, "znippy_rows_create failed");
    znippy_rows_set_blob_cap(*rt, blob_cap);
    return ZNIPPY_OK;
}

// "checksum mismatch" / "decompress failed" of the first row or range that has one
int sweep_status(const std::vector<int32_t> &st, const char *rel) {
    for (int32_t v : st) {
        if (v == ZNIPPY_E_DIGEST) return fail(ZNIPPY_E_CHECKSUM, std::string("checksum mismatch in ") + rel);
        if (v < 0) return fail(v, "OpenZL-equivalent decompress failed");
    }
    return ZNIPPY_OK;
}

// Blob bytes -> HBM -> decode+verify kernels; the decoded rows stay in bufs.d_out (the caller decides whether
// they cross PCIe at all).  Stands for the worker loop body, decompress.rs:L135-190.  keep_out = false (save_data=false,
// L186-189): no output region at all — the rows are checked by a verify-only run (znippy_verify_rows) and bufs.d_out is not touched.
// decode_only (with keep_out and without verify: the extract path, archive.rs:L144-168): a decode-only run (znippy_decode_rows) — nothing is hashed.
int decode_range(znippy_ctx *ctx, int arc_fd, const znippy_index &ix, const uint64_t *row_ids, size_t n, bool verify, ReadBufs &bufs,
                 DecodedRange *dr, bool keep_out = true, bool decode_only = false) {
    zn::RowsRead p = zn::plan_rows_read(ix.view(), row_ids, n, verify);
    if (p.rc) return fail(p.rc, p.err);
    dr->out_off.swap(p.out_off);
    dr->len = p.t.us;
    dr->total = p.total;
    dr->status.assign(n, 0);
    dr->cnt = znippy_verify_counters{};
    if (!n) return ZNIPPY_OK;
    double t = now_s();
    if (!bufs.blob_pin.reserve(p.nblob + 64)) return fail(ZNIPPY_E_NOMEM, "page-locked allocation failed");
    if (!read_into_slab(arc_fd, bufs.blob_pin.p, p.reads)) return fail(ZNIPPY_E_INVAL, "failed to read blob from archive");
    bufs.t_read += now_s() - t; t = now_s();
    if (!bufs.d_blobs.reserve(p.nblob + 64) || (keep_out && !bufs.d_out.reserve(dr->total + 64))) return fail(ZNIPPY_E_NOMEM, "device allocation failed");
    if (p.nblob && hipMemcpy(bufs.d_blobs.p, bufs.blob_pin.p, p.nblob, hipMemcpyHostToDevice) != hipSuccess) return fail(ZNIPPY_E_HIP, "H2D failed");
    bufs.t_h2d += now_s() - t; t = now_s();
    znippy_rows *rt = nullptr;
    int rc = create_rows(ctx, p.t, keep_out ? dr->out_off.data() : nullptr, p.nblob, &rt);
    if (rc) return rc;
    std::vector<uint64_t> cr(n);
    if (keep_out && decode_only && !verify) rc = znippy_decode_rows(ctx, rt, bufs.d_blobs.p, p.base, bufs.d_out.p, dr->total, &dr->cnt, dr->status.data());
    else if (keep_out) rc = znippy_decode_verify_rows(ctx, rt, bufs.d_blobs.p, p.base, bufs.d_out.p, dr->total, &dr->cnt, cr.data(), n, dr->status.data());
    else rc = znippy_verify_rows(ctx, rt, bufs.d_blobs.p, p.base, &dr->cnt, cr.data(), n, dr->status.data());
    znippy_rows_destroy(rt);
    if (rc) return fail(rc, std::string("decode failed: ") + znippy_last_error(ctx));
    bufs.t_kern += now_s() - t;
    for (uint64_t k = 0; k < dr->cnt.corrupt_rows && k < n; k++) dr->corrupt.push_back(row_ids[cr[k]]);
    return ZNIPPY_OK;
}

// Positioned writes of decoded rows [k0,k1) of one range (decompress.rs:L186-189).  A file is created (and,
// when this rank owns the whole archive, truncated) at its first row; rows of one file are adjacent, so one
// cached descriptor per writer replaces the reference's table of open files.
struct RowWriter {
    IndexView ix;
    const char *out_dir;
    const std::vector<uint8_t> *first_touch;
    bool truncate;  // this process owns the whole archive: O_TRUNC on first touch, like the reference (L74-101)
    const std::unordered_map<std::string, uint64_t> *final_size;  // several ranks share the files: first touch sets the final size (read_plan_first_touch)
    std::atomic<int> *err;
    void operator()(const uint8_t *bytes, const DecodedRange *dr, uint64_t row0, uint64_t k0, uint64_t k1) const {
        std::string cur_dir;
        const std::string *cur_path = nullptr;
        int fd = -1;
        for (uint64_t k = k0; k < k1; k++) {
            const uint64_t r = row0 + k;
            if (dr->status[k] < 0) {  // decode error: logged + skipped (L159-162)
                fprintf(stderr, "[decomp] row %llu error=%d\n", (unsigned long long)r, dr->status[k]);
                continue;
            }
            const std::string &p = ix.path[r];
            if (!cur_path || *cur_path != p) {
                if (fd >= 0) close(fd);
                const std::string full = std::string(out_dir) + "/" + p;
                const bool first = (*first_touch)[r] != 0;
                if (first) {
                    const std::string dir = full.substr(0, full.find_last_of('/'));
                    if (dir != cur_dir) { mkdirs(dir); cur_dir = dir; }
                }
                fd = open(full.c_str(), O_CREAT | O_WRONLY | ((first && truncate) ? O_TRUNC : 0), 0644);
                cur_path = &p;
                if (fd < 0) { err->store(1); g_open_failed(p); return; }
                if (first && !truncate && final_size) {
                    auto it = final_size->find(p);
                    if (it != final_size->end() && ftruncate(fd, (off_t)it->second) != 0) err->store(2);
                }
            }
            if (!pwrite_all(fd, bytes + dr->out_off[k], dr->len[k], ix.fdata_offset[r])) err->store(2);
        }
        if (fd >= 0) close(fd);
    }
    static void g_open_failed(const std::string &p) { fprintf(stderr, "[decomp] failed to open output file %s\n", p.c_str()); }
};

}  // namespace

extern "C" {

static int znippy_decompress_archive_impl(const char *index_path, int save_data, const char *out_dir, int device, uint32_t rank,
                              uint32_t world, znippy_verify_report *report, uint64_t *corrupt_rows, uint64_t corrupt_cap,
                              uint64_t *n_corrupt) {
    if (!index_path || !report || (save_data && !out_dir) || world == 0 || rank >= world) return fail(ZNIPPY_E_INVAL, "bad argument");
    const double t_begin = now_s();
    znippy_index ix;
    int rc = load_index(index_path, &ix);
    if (rc) return rc;
    const double t_index = now_s();
    const IndexView view = ix.view();
    const std::string *paths = view.path;
    const auto range = zn::split_rows(view.usize, view.n, rank, world);
    const zn::FirstTouch touch = zn::read_plan_first_touch(view, range.first, range.second, world > 1 && save_data);
    const size_t n_unique = touch.n_unique;
    if (save_data) mkdirs(out_dir);
    int arc = open(index_path, O_RDONLY);
    if (arc < 0) return fail(ZNIPPY_E_INVAL, "cannot open archive");
    znippy_ctx *ctx = nullptr;
    if (range.second > range.first) {
        if (hipSetDevice(device) != hipSuccess || (rc = znippy_ctx_create(device, nullptr, &ctx))) {
            close(arc);
            return fail(rc ? rc : ZNIPPY_E_HIP, "no usable GPU: the codec/hash path has no CPU fallback");
        }
    }
    const double t_ctx = now_s();
    znippy_verify_counters tot{};
    std::vector<uint64_t> corrupt;
    ReadBufs bufs;
    // save_data: the decoded range crosses PCIe into one of two page-locked slabs and a few writer threads
    // scatter it into the output files while the GPU works on the next range.  verify-only: nothing is copied back.
    struct OutSlab {
        PinBuf pin;
        DecodedRange dr;
        std::vector<std::thread> writers;
        uint64_t last_row = 0;
        void join() { for (auto &t : writers) t.join(); writers.clear(); }
    } slabs[2];
    std::atomic<int> werr{0};
    const RowWriter writer{view, out_dir, &touch.first, world == 1, world > 1 ? &touch.final_size : nullptr, &werr};
    const unsigned n_writers = touch.adjacent ? writer_threads() : 1;
    const uint64_t batch_bytes = range_bytes(save_data != 0);
    // save_data=false: rows are verified without being written (ZNIPPY_NO_VERIFY_ONLY=1 in the environment: decoded into a region
    // that is thrown away, as before — for A/B); cut_batch cuts such a range by what it takes on the device.
    const bool verify_only = !save_data && !env_on("ZNIPPY_NO_VERIFY_ONLY");
    double t_d2h = 0, t_wjoin = 0;
    int which = 0, n_ranges = 0;
    uint64_t i = range.first;
    std::vector<uint64_t> ids;
    while (i < range.second && rc == ZNIPPY_OK && !werr.load()) {
        const uint64_t j = zn::cut_batch(view, i, range.second, batch_bytes, verify_only);
        ids.resize(j - i);
        for (uint64_t k = i; k < j; k++) ids[k - i] = k;
        OutSlab &sl = slabs[which];
        double t = now_s();
        sl.join();  // the slab's previous range has been written out
        // a file continuing from the range still being written must see its first-touch create/truncate first
        OutSlab &other = slabs[which ^ 1];
        if (!other.writers.empty() && i && paths[i] == paths[i - 1]) other.join();
        t_wjoin += now_s() - t;
        sl.dr.corrupt.clear();
        rc = decode_range(ctx, arc, ix, ids.data(), ids.size(), true, bufs, &sl.dr, !verify_only);
        if (rc) break;
        n_ranges++;
        const znippy_verify_counters &c = sl.dr.cnt;
        tot.total_chunks += c.total_chunks; tot.total_written_bytes += c.total_written_bytes;
        tot.verified_bytes += c.verified_bytes; tot.corrupt_bytes += c.corrupt_bytes;
        tot.corrupt_rows += c.corrupt_rows; tot.decode_errors += c.decode_errors;
        corrupt.insert(corrupt.end(), sl.dr.corrupt.begin(), sl.dr.corrupt.end());
        if (save_data) {
            t = now_s();
            if (!sl.pin.reserve(sl.dr.total + 64)) { rc = fail(ZNIPPY_E_NOMEM, "page-locked allocation failed"); break; }
            if (sl.dr.total && hipMemcpy(sl.pin.p, bufs.d_out.p, sl.dr.total, hipMemcpyDeviceToHost) != hipSuccess) { rc = fail(ZNIPPY_E_HIP, "D2H failed"); break; }
            t_d2h += now_s() - t;
            for (const auto &part : zn::cut_writers(sl.dr.out_off.data(), sl.dr.total, paths, i, j - i, n_writers))
                sl.writers.emplace_back(writer, sl.pin.p, &sl.dr, i, part.first, part.second);
            which ^= 1;
        }
        i = j;
    }
    double t = now_s();
    slabs[0].join();
    slabs[1].join();
    t_wjoin += now_s() - t;
    close(arc);
    if (ctx) znippy_ctx_destroy(ctx);
    if (rc) return rc;
    if (werr.load()) return fail(ZNIPPY_E_INVAL, werr.load() == 1 ? "failed to open output file" : "failed to write output file");
    if (trace_on())
        fprintf(stderr, "[host] decompress_archive: index %.1f ms  ctx %.1f ms  ranges %d  pread %.1f ms  h2d %.1f ms  kernels %.1f ms  d2h %.1f ms  "
                        "writer-wait %.1f ms  total %.1f ms\n",
                (t_index - t_begin) * 1e3, (t_ctx - t_index) * 1e3, n_ranges, bufs.t_read * 1e3, bufs.t_h2d * 1e3, bufs.t_kern * 1e3, t_d2h * 1e3,
                t_wjoin * 1e3, (now_s() - t_begin) * 1e3);
    std::sort(corrupt.begin(), corrupt.end());
    for (uint64_t r : corrupt) fprintf(stderr, "[verify] MISMATCH row=%llu\n", (unsigned long long)r);
    const uint64_t corrupt_files = corrupt.size();  // number of corrupt ROWS (L210)
    report->total_files = n_unique;
    report->corrupt_files = corrupt_files;
    report->verified_files = n_unique > corrupt_files ? n_unique - corrupt_files : 0;
    report->total_bytes = tot.total_written_bytes;
    report->verified_bytes = tot.verified_bytes;
    report->corrupt_bytes = tot.corrupt_bytes;
    report->chunks = tot.total_chunks;
    if (n_corrupt) *n_corrupt = corrupt.size();
    if (corrupt_rows)
        for (uint64_t k = 0; k < corrupt.size() && k < corrupt_cap; k++) corrupt_rows[k] = corrupt[k];
    return ZNIPPY_OK;
}

// ---- ZnippyArchive ------------------------------------------------------------------------------
}  // extern "C"

struct znippy_archive {
    std::string path;
    int device = 0;
    znippy_index ix;
    std::unordered_map<std::string, std::vector<uint64_t>> files;  // rows sorted by fdata_offset (archive.rs:L131-133)
    znippy_ctx *ctx = nullptr;
    int fd = -1;
    ReadBufs bufs;
    // verified range reads: archive row -> the entries of its block tree (32 bytes per 128 KiB block), built once per chunk by a whole
    // decode with a root check and authenticated again, against the index checksum, by every read that installs them
    std::unordered_map<uint64_t, std::vector<uint8_t>> block_trees;
    // the sidecar `<path>.b3t`, if one was there at open and agrees with the index: the entries of all rows and where each row's start.
    // Untrusted — a chunk's entries enter block_trees only once znippy_rows_set_block_tree has accepted them against the index checksum
    std::vector<uint8_t> side_tree;
    std::vector<uint64_t> side_first;  // n + 1 values; empty: no usable sidecar
    uint64_t tree_stats[4] = {0, 0, 0, 0};  // znippy_archive_block_tree_stats
};

namespace {
// A sidecar that is missing, malformed, or disagrees with the index in n_rows or n_entries is ignored (zn::sidecar_layout).
void load_sidecar(znippy_archive *a) {
    const std::string path = a->path + ".b3t";
    const int fd = open(path.c_str(), O_RDONLY);
    if (fd < 0) return;
    struct stat st;
    std::vector<uint8_t> raw;
    const bool ok = fstat(fd, &st) == 0 && (raw.resize((size_t)st.st_size), pread_all(fd, raw.data(), raw.size(), 0));
    close(fd);
    std::vector<uint64_t> first;
    if (!ok || !zn::sidecar_layout(raw.data(), raw.size(), a->ix.view(), &first)) return;
    a->side_tree.assign(raw.begin() + B3T_HEADER, raw.end());
    a->tree_stats[0] = first.back();
    a->side_first.swap(first);
}

int archive_ctx(znippy_archive *a) {  // the context is created at the first call that needs the GPU
    if (a->ctx) return ZNIPPY_OK;
    if (hipSetDevice(a->device) != hipSuccess) return fail(ZNIPPY_E_HIP, "hipSetDevice failed");
    const int rc = znippy_ctx_create(a->device, nullptr, &a->ctx);
    return rc ? fail(rc, "no usable GPU: the codec/hash path has no CPU fallback") : ZNIPPY_OK;
}

// Verified range reads: rows `fresh` of the read's table t (table row k is archive row arow[k]) have entries and no cached tree yet.
// First the sidecar's entries for them are offered — as one private table over the same slab — and cached without any decode where
// znippy_rows_set_block_tree accepts them against the index checksum; *fresh becomes the rows it refused.
int offer_sidecar(znippy_archive *a, const RowTable &t, const std::vector<uint64_t> &arow, std::vector<size_t> *fresh) {
    const RowTable ft = t.subset(*fresh);
    std::vector<uint8_t> tree;
    for (size_t k : *fresh) {  // (the sidecar's layout was checked against the index: this row has tree_entries_of(us[k]) there)
        const uint64_t *first = &a->side_first[arow[k]];
        zn::take_tree(a->side_tree.data(), 32 * (size_t)first[0], first[1] - first[0], &tree);
    }
    znippy_rows *bt = nullptr;
    int rc = create_rows(a->ctx, ft, nullptr, ~0ull, &bt);
    if (rc) return rc;
    std::vector<int32_t> bst(ft.n(), 0);
    rc = znippy_rows_set_block_tree(a->ctx, bt, tree.data(), bst.data());
    znippy_rows_destroy(bt);
    if (rc) return fail(rc, std::string("block tree check failed: ") + znippy_last_error(a->ctx));
    std::vector<size_t> rest;
    size_t at = 0;
    for (size_t i = 0; i < ft.n(); i++) {
        std::vector<uint8_t> entries;
        at = zn::take_tree(tree.data(), at, zn::tree_entries_of(ft.us[i]), &entries);
        if (bst[i] == 0) {
            a->block_trees[arow[(*fresh)[i]]] = std::move(entries);
            a->tree_stats[1]++;
        } else {  // rejected: the whole-decode build
            rest.push_back((*fresh)[i]);
            a->tree_stats[2]++;
        }
    }
    fresh->swap(rest);
    return ZNIPPY_OK;
}

// ... the rest is built: one private table, one whole decode of its rows (their blobs are in bufs.d_blobs) whose digests must be
// the index checksums.
int build_trees(znippy_archive *a, const RowTable &t, const std::vector<uint64_t> &arow, const std::vector<size_t> &fresh, const char *rel) {
    const RowTable ft = t.subset(fresh);
    uint64_t n_entries = 0;
    for (uint64_t us : ft.us) n_entries += zn::tree_entries_of(us);
    znippy_rows *bt = nullptr;
    int rc = create_rows(a->ctx, ft, nullptr, ft.sum, &bt);
    if (rc) return rc;
    std::vector<uint8_t> tree(32 * (size_t)n_entries);
    std::vector<int32_t> bst(ft.n(), 0);
    rc = znippy_rows_block_tree_build(a->ctx, bt, a->bufs.d_blobs.p, 0, tree.data(), bst.data());
    znippy_rows_destroy(bt);
    if (rc) return fail(rc, std::string("block tree build failed: ") + znippy_last_error(a->ctx));
    if ((rc = sweep_status(bst, rel))) return rc;
    size_t at = 0;
    for (size_t i = 0; i < ft.n(); i++) {
        at = zn::take_tree(tree.data(), at, zn::tree_entries_of(ft.us[i]), &a->block_trees[arow[fresh[i]]]);
        a->tree_stats[3]++;
    }
    return ZNIPPY_OK;
}
}  // namespace


extern "C" {

static int znippy_archive_open_impl(const char *path, int device, znippy_archive **out) {
    if (!path || !out) return fail(ZNIPPY_E_INVAL, "null argument");
    std::unique_ptr<znippy_archive> a(new znippy_archive());
    a->path = path;
    a->device = device;
    int rc = load_index(path, &a->ix);
    if (rc) return rc;
    const IndexView v = a->ix.view();
    for (uint64_t r = 0; r < v.n; r++) a->files[v.path[r]].push_back(r);
    for (auto &kv : a->files)
        std::stable_sort(kv.second.begin(), kv.second.end(), [&](uint64_t x, uint64_t y) { return v.fdata_offset[x] < v.fdata_offset[y]; });
    a->fd = open(path, O_RDONLY);
    if (a->fd < 0) return fail(ZNIPPY_E_INVAL, "cannot open archive");
    load_sidecar(a.get());
    *out = a.release();
    return ZNIPPY_OK;
}

uint64_t znippy_archive_file_count(const znippy_archive *a) { return a ? a->files.size() : 0; }

int64_t znippy_archive_file_size(const znippy_archive *a, const char *rel) {
    if (!a || !rel) return -1;
    auto it = a->files.find(rel);
    if (it == a->files.end()) return -1;
    uint64_t s = 0;
    for (uint64_t r : it->second) s += a->ix.view().usize[r];
    return (int64_t)s;
}

static int znippy_archive_extract_file_impl(znippy_archive *a, const char *rel, void *dst, size_t cap, size_t *written, int verify = 0) {
    if (!a || !rel || !written) return fail(ZNIPPY_E_INVAL, "null argument");
    auto it = a->files.find(rel);
    if (it == a->files.end()) return fail(ZNIPPY_E_INVAL, std::string("file not found in archive: ") + rel);
    int rc = archive_ctx(a);
    if (rc) return rc;
    DecodedRange dr;
    // the unverified extract hashes nothing (ZNIPPY_NO_DECODE_ONLY=1 in the environment: the decode + verify run without a checksum
    // column, as before — for A/B runs)
    const bool decode_only = !verify && !env_on("ZNIPPY_NO_DECODE_ONLY");
    rc = decode_range(a->ctx, a->fd, a->ix, it->second.data(), it->second.size(), verify != 0, a->bufs, &dr, true, decode_only);
    if (rc) return rc;
    for (int32_t st : dr.status)
        if (st < 0) return fail(st, "OpenZL-equivalent decompress failed");  // propagates (archive.rs:L160)
    // optional verify (the reference's extract_file has none, archive.rs:L144-168; SURVEY §8f rank 1 adds it): every
    // chunk's BLAKE3 against the index's checksum column, computed by the same kernels as the bulk path
    if (verify && dr.cnt.corrupt_rows) return fail(ZNIPPY_E_CHECKSUM, std::string("checksum mismatch in ") + rel);
    if (dr.total > cap) return fail(ZNIPPY_E_DST_SMALL, "destination too small");
    if (dr.total && hipMemcpy(dst, a->bufs.d_out.p, dr.total, hipMemcpyDeviceToHost) != hipSuccess) return fail(ZNIPPY_E_HIP, "D2H failed");
    *written = dr.total;
    return ZNIPPY_OK;
}

// pread on an archived file (ZnippyArchive.read_range in archive.py): the range is mapped to the chunks it touches by fdata_offset, only
// their blobs are read from the archive, and znippy_rows_read_ranges decodes no more of them than the range needs.
// verify: znippy_archive_read_range_verified — the small table gets the chunks' checksums and their cached block trees, and the read is
// znippy_rows_read_ranges_verified.  A chunk with entries that is touched for the first time is built once (a whole decode whose digest
// must be the index checksum); afterwards a read hashes only the 128 KiB blocks it returns bytes of.  The blobs come from the file on
// every call, so damage that appears between two reads is caught for the blocks a read touches.
static int znippy_archive_read_range_impl(znippy_archive *a, const char *rel, uint64_t offset, void *dst, size_t len, size_t *written, int verify = 0) {
    if (!a || !rel || !written || (len && !dst)) return fail(ZNIPPY_E_INVAL, "null argument");
    *written = 0;
    auto it = a->files.find(rel);
    if (it == a->files.end()) return fail(ZNIPPY_E_INVAL, std::string("file not found in archive: ") + rel);
    const zn::RangeRead p = zn::plan_range_read(a->ix.view(), it->second.data(), it->second.size(), offset, len, verify != 0);
    if (p.rc) return fail(p.rc, "blob range outside the archive");
    const RowTable &t = p.t;
    if (!t.n()) return ZNIPPY_OK;  // at or past the end of the file, or an empty range
    int rc = archive_ctx(a);
    if (rc) return rc;
    ReadBufs &bufs = a->bufs;
    if (!bufs.blob_pin.reserve(std::max<uint64_t>(t.sum, p.total) + 64)) return fail(ZNIPPY_E_NOMEM, "page-locked allocation failed");
    if (!read_into_slab(a->fd, bufs.blob_pin.p, t.reads())) return fail(ZNIPPY_E_INVAL, "failed to read blob from archive");
    if (!bufs.d_blobs.reserve(t.sum + 64) || !bufs.d_out.reserve(p.total + 64)) return fail(ZNIPPY_E_NOMEM, "device allocation failed");
    if (t.sum && hipMemcpy(bufs.d_blobs.p, bufs.blob_pin.p, t.sum, hipMemcpyHostToDevice) != hipSuccess) return fail(ZNIPPY_E_HIP, "H2D failed");
    if (verify) {  // chunks with entries that this handle has not built yet
        std::vector<size_t> fresh;
        for (size_t k = 0; k < t.n(); k++)
            if (zn::tree_entries_of(t.us[k]) && !a->block_trees.count(p.arow[k])) fresh.push_back(k);
        if (!fresh.empty() && !a->side_first.empty()) rc = offer_sidecar(a, t, p.arow, &fresh);
        if (!rc && !fresh.empty()) rc = build_trees(a, t, p.arow, fresh, rel);
        if (rc) return rc;
    }
    znippy_rows *rt = nullptr;
    rc = create_rows(a->ctx, t, nullptr, t.sum, &rt);
    if (rc) return rc;
    const zn::RangeList &rg = p.rg;
    std::vector<int32_t> st(rg.n(), 0);
    if (verify) {
        std::vector<uint8_t> tree;  // the tree of this table: its rows' cached entries, in row order
        for (uint64_t r : p.arow) {
            auto bt = a->block_trees.find(r);
            if (bt != a->block_trees.end()) zn::take_tree(bt->second.data(), 0, bt->second.size() / 32, &tree);
        }
        tree.push_back(0);  // (never NULL: that would remove the tree)
        rc = znippy_rows_set_block_tree(a->ctx, rt, tree.data(), nullptr);
        if (!rc) rc = znippy_rows_read_ranges_verified(a->ctx, rt, bufs.d_blobs.p, 0, rg.row.data(), rg.begin.data(), rg.len.data(), nullptr, rg.n(), bufs.d_out.p, p.total, st.data(), nullptr, nullptr);
    } else
        rc = znippy_rows_read_ranges(a->ctx, rt, bufs.d_blobs.p, 0, rg.row.data(), rg.begin.data(), rg.len.data(), nullptr, rg.n(), bufs.d_out.p, p.total, st.data(), nullptr);
    znippy_rows_destroy(rt);
    if (rc) return fail(rc, std::string("range read failed: ") + znippy_last_error(a->ctx));
    if ((rc = sweep_status(st, rel))) return rc;
    if (hipMemcpy(dst, bufs.d_out.p, p.total, hipMemcpyDeviceToHost) != hipSuccess) return fail(ZNIPPY_E_HIP, "D2H failed");
    *written = p.total;
    return ZNIPPY_OK;
}

}  // extern "C"

// ---- entries of archived ZIP containers (znippy_archive_extract_zip_entries) ----------------------------
namespace {

using zn::FileRange;  // bytes [off, off + len) of one archived file, wholly inside it

// One range-read pass for many files (zn::plan_file_ranges): the planned blobs are read from the archive and uploaded in one copy,
// ONE znippy_rows_read_ranges over a private table of them gathers all requests packed back to back, and one copy brings them to the
// host: request i at host[at[i] .. at[i] + len), st[i] = 0 or a chunk's ZNIPPY_E_*.  Nothing is kept between passes: a compressed
// chunk that two passes touch is read and uploaded twice.
// host == NULL: the copy to the host is skipped and the requests stay on the device, request i at a->bufs.d_out.p + at[i], *on_device
// bytes in all (for a caller that goes on working on them there).
int read_file_ranges(znippy_archive *a, const std::vector<FileRange> &req, std::vector<uint8_t> *host, std::vector<uint64_t> *at,
                     std::vector<int32_t> *st, uint64_t *on_device = nullptr) {
    zn::FileRangesRead p = zn::plan_file_ranges(a->ix.view(), req);
    const RowTable &t = p.t;
    const zn::RangeList &rg = p.rg;
    const uint64_t total = p.total;
    at->swap(p.at);
    st->swap(p.st);
    if (host) host->assign((size_t)total, 0);
    if (on_device) *on_device = total;
    if (!rg.n()) return ZNIPPY_OK;
    ReadBufs &bufs = a->bufs;
    if (!bufs.blob_pin.reserve(std::max<uint64_t>(t.sum, total) + 64)) return fail(ZNIPPY_E_NOMEM, "page-locked allocation failed");
    if (!read_into_slab(a->fd, bufs.blob_pin.p, t.reads())) return fail(ZNIPPY_E_INVAL, "failed to read blob from archive");
    if (!bufs.d_blobs.reserve(t.sum + 64) || !bufs.d_out.reserve(total + 64)) return fail(ZNIPPY_E_NOMEM, "device allocation failed");
    if (t.sum && hipMemcpy(bufs.d_blobs.p, bufs.blob_pin.p, t.sum, hipMemcpyHostToDevice) != hipSuccess) return fail(ZNIPPY_E_HIP, "H2D failed");
    znippy_rows *rt = nullptr;
    int rc = create_rows(a->ctx, t, nullptr, t.sum, &rt);
    if (rc) return rc;
    std::vector<int32_t> rst(rg.n(), 0);
    rc = znippy_rows_read_ranges(a->ctx, rt, bufs.d_blobs.p, 0, rg.row.data(), rg.begin.data(), rg.len.data(), nullptr, rg.n(), bufs.d_out.p, total, rst.data(), nullptr);
    znippy_rows_destroy(rt);
    if (rc) return fail(rc, std::string("range read failed: ") + znippy_last_error(a->ctx));
    for (size_t k = 0; k < rst.size(); k++)
        if (rst[k] < 0 && (*st)[p.of_req[k]] == 0) (*st)[p.of_req[k]] = rst[k];
    if (host && total && hipMemcpy(host->data(), bufs.d_out.p, total, hipMemcpyDeviceToHost) != hipSuccess) return fail(ZNIPPY_E_HIP, "D2H failed");
    return ZNIPPY_OK;
}

}  // namespace

static int znippy_archive_extract_zip_entries_impl(znippy_archive *a, const char *const *paths, uint64_t n_files, const char *name_prefix,
                                                   const char *name_suffix, void *dst, size_t cap, uint64_t *entry_off, int32_t *status) {
    if (!a || !entry_off || (n_files && !paths) || (cap && !dst)) return fail(ZNIPPY_E_INVAL, "null argument");
    const char *prefix = name_prefix ? name_prefix : "", *suffix = name_suffix ? name_suffix : "";
    const size_t n = (size_t)n_files;
    std::vector<int32_t> st(n, 0);
    std::vector<const std::vector<uint64_t> *> rows(n, nullptr);
    std::vector<uint64_t> fsize(n, 0);
    const IndexView view = a->ix.view();
    for (size_t i = 0; i < n; i++) {
        auto it = paths[i] ? a->files.find(paths[i]) : a->files.end();
        if (it == a->files.end()) { st[i] = ZNIPPY_E_INVAL; continue; }
        rows[i] = &it->second;
        for (uint64_t r : it->second) fsize[i] += view.row_len(r);
    }
    int rc = archive_ctx(a);
    if (rc) return rc;
    std::vector<FileRange> req;
    std::vector<size_t> who;  // request -> file
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> at;
    std::vector<int32_t> rst;
    auto pass = [&]() -> int {
        const int rc = read_file_ranges(a, req, &bytes, &at, &rst);
        if (!rc)
            for (size_t k = 0; k < req.size(); k++)
                if (rst[k] && st[who[k]] == 0) st[who[k]] = rst[k];
        return rc;
    };
    // 1) the tails: where each container's central directory is
    std::vector<uint64_t> dir_off(n, 0), dir_size(n, 0), dir_n(n, 0);
    for (size_t i = 0; i < n; i++) {
        if (st[i] == 0 && fsize[i] < 22) st[i] = ZNIPPY_E_CORRUPT;  // no room for an end record
        if (st[i]) continue;
        const uint64_t tl = std::min<uint64_t>(fsize[i], ZN_ZIP_TAIL_MAX);
        req.push_back(FileRange{rows[i], fsize[i] - tl, tl});
        who.push_back(i);
    }
    rc = pass();
    if (rc) return rc;
    for (size_t k = 0; k < req.size(); k++) {
        const size_t i = who[k];
        if (st[i] == 0) st[i] = znippy_zip_end_of_directory(bytes.data() + at[k], (size_t)req[k].len, fsize[i], &dir_off[i], &dir_size[i], &dir_n[i]);
    }
    // 2) the central directories: the first entry that matches
    std::vector<znippy_zip_entry> ent(n);
    req.clear(); who.clear();
    for (size_t i = 0; i < n; i++) {
        if (st[i]) continue;
        req.push_back(FileRange{rows[i], dir_off[i], dir_size[i]});
        who.push_back(i);
    }
    rc = pass();
    if (rc) return rc;
    for (size_t k = 0; k < req.size(); k++) {
        const size_t i = who[k];
        if (st[i]) continue;
        st[i] = znippy_zip_find_entry(bytes.data() + at[k], (size_t)req[k].len, dir_n[i], prefix, strlen(prefix), suffix, strlen(suffix), &ent[i]);
        if (st[i] == 0 && ent[i].method > 255) st[i] = ZNIPPY_E_UNSUPPORTED;
        // the entry lies in front of the directory: its fixed header at least, and then its data
        if (st[i] == 0 && (ent[i].local_header_offset > dir_off[i] || dir_off[i] - ent[i].local_header_offset < 30 + ent[i].compressed_size)) st[i] = ZNIPPY_E_CORRUPT;
    }
    // 3) local header + compressed bytes.  The name and extra lengths that place the data are the LOCAL header's, unknown until it is
    //    read: the request runs to the farthest place they can put the end of the data, or to the directory if that comes first
    req.clear(); who.clear();
    for (size_t i = 0; i < n; i++) {
        if (st[i]) continue;
        const uint64_t lho = ent[i].local_header_offset, reach = 30 + 2 * 65535ull + ent[i].compressed_size;
        req.push_back(FileRange{rows[i], lho, std::min(reach, dir_off[i] - lho)});
        who.push_back(i);
    }
    rc = pass();
    if (rc) return rc;
    // 4) the compressed streams, packed, in one upload
    std::vector<uint64_t> s_off, s_len, u_len, u_off;
    std::vector<uint8_t> method;
    std::vector<uint32_t> crc;
    std::vector<size_t> item_file;
    uint64_t c_total = 0, u_total = 0;
    std::vector<std::pair<uint64_t, uint64_t>> where;  // item -> (position in `bytes`, length)
    for (size_t k = 0; k < req.size(); k++) {
        const size_t i = who[k];
        if (st[i]) continue;
        uint64_t data_off = 0;
        st[i] = znippy_zip_local_data_offset(bytes.data() + at[k], (size_t)std::min<uint64_t>(req[k].len, 30), &data_off);
        if (st[i] == 0 && (data_off > req[k].len || req[k].len - data_off < ent[i].compressed_size)) st[i] = ZNIPPY_E_CORRUPT;
        if (st[i]) continue;
        where.emplace_back(at[k] + data_off, ent[i].compressed_size);
        s_off.push_back(c_total); s_len.push_back(ent[i].compressed_size); u_off.push_back(u_total); u_len.push_back(ent[i].uncompressed_size);
        method.push_back((uint8_t)ent[i].method); crc.push_back(ent[i].crc32); item_file.push_back(i);
        c_total += ent[i].compressed_size;
        u_total += ent[i].uncompressed_size;
    }
    ReadBufs &bufs = a->bufs;
    if (!item_file.empty()) {
        if (!bufs.blob_pin.reserve(std::max(c_total, u_total) + 64) || !bufs.d_blobs.reserve(c_total + 64) || !bufs.d_out.reserve(u_total + 64))
            return fail(ZNIPPY_E_NOMEM, "allocation failed");
        for (size_t j = 0; j < where.size(); j++)
            if (where[j].second) std::memcpy(bufs.blob_pin.p + s_off[j], bytes.data() + where[j].first, (size_t)where[j].second);
        if (c_total && hipMemcpy(bufs.d_blobs.p, bufs.blob_pin.p, c_total, hipMemcpyHostToDevice) != hipSuccess) return fail(ZNIPPY_E_HIP, "H2D failed");
        // 5) one inflate over all of them, against the directory's CRCs
        std::vector<int32_t> ist(item_file.size(), 0);
        rc = znippy_inflate_batch(a->ctx, bufs.d_blobs.p, c_total, s_off.data(), s_len.data(), method.data(), bufs.d_out.p, u_total, nullptr, u_len.data(),
                                  crc.data(), item_file.size(), ist.data(), nullptr);
        if (rc) return fail(rc, std::string("inflate failed: ") + znippy_last_error(a->ctx));
        for (size_t j = 0; j < item_file.size(); j++) st[item_file[j]] = ist[j];
        // 6) one copy back
        if (u_total && hipMemcpy(bufs.blob_pin.p, bufs.d_out.p, u_total, hipMemcpyDeviceToHost) != hipSuccess) return fail(ZNIPPY_E_HIP, "D2H failed");
    }
    // the contents, packed in file order; a file that does not fit is left out and the ones behind it may still fit
    std::vector<uint64_t> item_of(n, UINT64_MAX);
    for (size_t j = 0; j < item_file.size(); j++) item_of[item_file[j]] = j;
    uint64_t cursor = 0;
    for (size_t i = 0; i < n; i++) {
        entry_off[i] = cursor;
        if (st[i] || item_of[i] == UINT64_MAX) continue;
        const uint64_t j = item_of[i], len = u_len[j];
        if (len > cap - cursor) { st[i] = ZNIPPY_E_DST_SMALL; continue; }
        if (len) std::memcpy((uint8_t *)dst + cursor, bufs.blob_pin.p + u_off[j], (size_t)len);
        cursor += len;
    }
    entry_off[n] = cursor;
    if (status) std::memcpy(status, st.data(), sizeof(int32_t) * n);
    return ZNIPPY_OK;
}

// ---- one member of archived gzip-compressed tars (znippy_archive_extract_tar_members) ----------------------------
// Pass 1 gathers the first `head` bytes of every file on the device (one range read, no copy to the host) and runs
// znippy_targz_find_batch on them there; pass 2 does the same with the whole file for exactly the files whose head did not hold the
// answer (ZNIPPY_E_MORE).  Only the members come back to the host.
static int znippy_archive_extract_tar_members_impl(znippy_archive *a, const char *const *paths, uint64_t n_files, const char *name_prefix,
                                                   const char *name_suffix, uint64_t scan_cap, void *dst, size_t cap, uint64_t *entry_off, int32_t *status) {
    if (!a || !entry_off || (n_files && !paths) || (cap && !dst) || scan_cap < 512) return fail(ZNIPPY_E_INVAL, "null argument or scan_cap below 512");
    const char *prefix = name_prefix ? name_prefix : "", *suffix = name_suffix ? name_suffix : "";
    uint64_t head = 64 << 10;
    if (const char *v = getenv("ZNIPPY_HOST_TARGZ_HEAD")) {  // (read at the call)
        char *end = nullptr;
        const unsigned long long h = strtoull(v, &end, 0);
        if (end != v && *end == 0 && h) head = h;
    }
    const size_t n = (size_t)n_files;
    std::vector<int32_t> st(n, 0);
    std::vector<const std::vector<uint64_t> *> rows(n, nullptr);
    std::vector<uint64_t> fsize(n, 0);
    const IndexView view = a->ix.view();
    for (size_t i = 0; i < n; i++) {
        auto it = paths[i] ? a->files.find(paths[i]) : a->files.end();
        if (it == a->files.end()) { st[i] = ZNIPPY_E_INVAL; continue; }
        rows[i] = &it->second;
        for (uint64_t r : it->second) fsize[i] += view.row_len(r);
        if (fsize[i] >= (1ull << 32)) st[i] = ZNIPPY_E_UNSUPPORTED;
        else if (fsize[i] == 0) st[i] = ZNIPPY_E_CORRUPT;  // no gzip member
    }
    int rc = archive_ctx(a);
    if (rc) return rc;
    std::vector<std::vector<uint8_t>> member(n);
    ReadBufs &bufs = a->bufs;
    // one pass over the files of `who`, the first take(i) bytes of each
    auto pass = [&](const std::vector<size_t> &who, bool whole_files) -> int {
        if (who.empty()) return ZNIPPY_OK;
        std::vector<FileRange> req;
        for (size_t i : who) req.push_back(FileRange{rows[i], 0, whole_files ? fsize[i] : std::min(fsize[i], head)});
        std::vector<uint64_t> at;
        std::vector<int32_t> rst;
        uint64_t total = 0;
        int rc = read_file_ranges(a, req, nullptr, &at, &rst, &total);
        if (rc) return rc;
        std::vector<uint64_t> s_off, s_len;
        std::vector<uint8_t> whole;
        std::vector<size_t> item_file;
        uint64_t bound = 0;  // what the members of this pass can come to
        for (size_t k = 0; k < who.size(); k++) {
            const size_t i = who[k];
            if (rst[k]) { st[i] = rst[k]; continue; }
            s_off.push_back(at[k]); s_len.push_back(req[k].len); whole.push_back(req[k].len == fsize[i]); item_file.push_back(i);
            bound += std::min<uint64_t>(scan_cap, 1032 * req[k].len + 512);
        }
        if (item_file.empty()) return ZNIPPY_OK;
        const uint64_t out_cap = std::min<uint64_t>(bound, cap);
        if (!bufs.d_blobs.reserve(out_cap + 64)) return fail(ZNIPPY_E_NOMEM, "device allocation failed");  // (the chunks in it have been gathered from)
        std::vector<uint64_t> o_off(item_file.size(), 0), o_len(item_file.size(), 0);
        std::vector<int32_t> ist(item_file.size(), 0);
        rc = znippy_targz_find_batch(a->ctx, bufs.d_out.p, total, s_off.data(), s_len.data(), whole.data(), item_file.size(), prefix, strlen(prefix), suffix,
                                     strlen(suffix), scan_cap, bufs.d_blobs.p, out_cap, o_off.data(), o_len.data(), ist.data(), nullptr);
        if (rc) return fail(rc, std::string("tar member search failed: ") + znippy_last_error(a->ctx));
        uint64_t found = 0;
        for (size_t j = 0; j < item_file.size(); j++) found = std::max(found, o_off[j] + o_len[j]);
        if (!bufs.blob_pin.reserve(found + 64)) return fail(ZNIPPY_E_NOMEM, "page-locked allocation failed");
        if (found && hipMemcpy(bufs.blob_pin.p, bufs.d_blobs.p, found, hipMemcpyDeviceToHost) != hipSuccess) return fail(ZNIPPY_E_HIP, "D2H failed");
        for (size_t j = 0; j < item_file.size(); j++) {
            st[item_file[j]] = ist[j];
            if (ist[j] == 0) member[item_file[j]].assign(bufs.blob_pin.p + o_off[j], bufs.blob_pin.p + o_off[j] + o_len[j]);
        }
        return ZNIPPY_OK;
    };
    std::vector<size_t> who;
    for (size_t i = 0; i < n; i++)
        if (st[i] == 0) who.push_back(i);
    if ((rc = pass(who, false))) return rc;
    who.clear();
    for (size_t i = 0; i < n; i++)
        if (st[i] == ZNIPPY_E_MORE) { st[i] = 0; who.push_back(i); }
    if ((rc = pass(who, true))) return rc;
    // the members, packed in file order; one that does not fit is left out and the ones behind it may still fit
    uint64_t cursor = 0;
    for (size_t i = 0; i < n; i++) {
        entry_off[i] = cursor;
        if (st[i]) continue;
        const uint64_t len = member[i].size();
        if (len > cap - cursor) { st[i] = ZNIPPY_E_DST_SMALL; continue; }
        if (len) std::memcpy((uint8_t *)dst + cursor, member[i].data(), (size_t)len);
        cursor += len;
    }
    entry_off[n] = cursor;
    if (status) std::memcpy(status, st.data(), sizeof(int32_t) * n);
    return ZNIPPY_OK;
}

// ---- the content of archived gzip files (znippy_archive_gunzip_files) ----------------------------
// Pass 1 reads the last four bytes of every file (ISIZE: exact for a file of one member); pass 2 gathers the files whole on the device
// (one range read, no copy to the host) and runs znippy_gunzip_batch on them there with those rooms.  The files that report
// ZNIPPY_E_DST_SMALL — several members, of which ISIZE names only the last — go through the call again with eight times the room,
// until they fit or the room is what DEFLATE can expand the file to.  Only the contents come back to the host.
static int znippy_archive_gunzip_files_impl(znippy_archive *a, const char *const *paths, uint64_t n_files, void *dst, size_t cap, uint64_t *entry_off,
                                            int32_t *status) {
    if (!a || !entry_off || (n_files && !paths) || (cap && !dst)) return fail(ZNIPPY_E_INVAL, "null argument");
    const size_t n = (size_t)n_files;
    std::vector<int32_t> st(n, 0);
    std::vector<const std::vector<uint64_t> *> rows(n, nullptr);
    std::vector<uint64_t> fsize(n, 0), room(n, 0);
    const IndexView view = a->ix.view();
    for (size_t i = 0; i < n; i++) {
        auto it = paths[i] ? a->files.find(paths[i]) : a->files.end();
        if (it == a->files.end()) { st[i] = ZNIPPY_E_INVAL; continue; }
        rows[i] = &it->second;
        for (uint64_t r : it->second) fsize[i] += view.row_len(r);
        if (fsize[i] >= (1ull << 32)) st[i] = ZNIPPY_E_UNSUPPORTED;
    }
    int rc = archive_ctx(a);
    if (rc) return rc;
    // 1) the rooms
    {
        std::vector<FileRange> req;
        std::vector<size_t> who;
        for (size_t i = 0; i < n; i++)
            if (st[i] == 0 && fsize[i] >= 4) { req.push_back(FileRange{rows[i], fsize[i] - 4, 4}); who.push_back(i); }
        std::vector<uint8_t> bytes;
        std::vector<uint64_t> at;
        std::vector<int32_t> rst;
        if ((rc = read_file_ranges(a, req, &bytes, &at, &rst))) return rc;
        for (size_t k = 0; k < req.size(); k++) {
            const uint8_t *p = bytes.data() + at[k];
            if (rst[k]) st[who[k]] = rst[k];
            else room[who[k]] = (uint64_t)p[0] | (uint64_t)p[1] << 8 | (uint64_t)p[2] << 16 | (uint64_t)p[3] << 24;
        }
    }
    // 2) the files, whole, on the device
    std::vector<size_t> who;
    std::vector<FileRange> req;
    for (size_t i = 0; i < n; i++)
        if (st[i] == 0) { who.push_back(i); req.push_back(FileRange{rows[i], 0, fsize[i]}); }
    std::vector<std::vector<uint8_t>> content(n);
    if (!who.empty()) {
        std::vector<uint64_t> at;
        std::vector<int32_t> rst;
        uint64_t total = 0;
        if ((rc = read_file_ranges(a, req, nullptr, &at, &rst, &total))) return rc;
        ReadBufs &bufs = a->bufs;
        std::vector<size_t> todo;  // indexes into who
        for (size_t k = 0; k < who.size(); k++) {
            if (rst[k]) st[who[k]] = rst[k];
            else todo.push_back(k);
        }
        // no valid DEFLATE expands more than 1032 : 1, and the call takes rooms below 4 GiB
        auto most = [&](size_t i) { return std::min<uint64_t>(1032 * fsize[i] + 512, 0xFFFFFFF0ull); };
        while (!todo.empty()) {
            std::vector<uint64_t> s_off, s_len, o_room, o_len(todo.size(), 0);
            uint64_t out_total = 0;
            for (size_t k : todo) {
                const size_t i = who[k];
                room[i] = std::min(room[i], most(i));
                s_off.push_back(at[k]); s_len.push_back(fsize[i]); o_room.push_back(room[i]);
                out_total += room[i];
            }
            if (!bufs.d_blobs.reserve(out_total + 64)) return fail(ZNIPPY_E_NOMEM, "device allocation failed");  // (the chunks in it have been gathered from)
            std::vector<int32_t> ist(todo.size(), 0);
            rc = znippy_gunzip_batch(a->ctx, bufs.d_out.p, total, s_off.data(), s_len.data(), todo.size(), bufs.d_blobs.p, out_total, nullptr, o_room.data(), 0,
                                     o_len.data(), ist.data(), nullptr, nullptr);
            if (rc) return fail(rc, std::string("gunzip failed: ") + znippy_last_error(a->ctx));
            if (!bufs.blob_pin.reserve(out_total + 64)) return fail(ZNIPPY_E_NOMEM, "page-locked allocation failed");
            if (out_total && hipMemcpy(bufs.blob_pin.p, bufs.d_blobs.p, out_total, hipMemcpyDeviceToHost) != hipSuccess) return fail(ZNIPPY_E_HIP, "D2H failed");
            std::vector<size_t> again;
            uint64_t o = 0;
            for (size_t j = 0; j < todo.size(); j++) {
                const size_t i = who[todo[j]];
                st[i] = ist[j];
                if (ist[j] == 0) content[i].assign(bufs.blob_pin.p + o, bufs.blob_pin.p + o + o_len[j]);
                else if (ist[j] == ZNIPPY_E_DST_SMALL && room[i] < most(i)) {
                    room[i] = std::max<uint64_t>(8 * room[i], 4096);
                    again.push_back(todo[j]);
                }
                o += o_room[j];
            }
            todo.swap(again);
        }
    }
    // the contents, packed in file order; one that does not fit is left out and the ones behind it may still fit
    uint64_t cursor = 0;
    for (size_t i = 0; i < n; i++) {
        entry_off[i] = cursor;
        if (st[i]) continue;
        const uint64_t len = content[i].size();
        if (len > cap - cursor) { st[i] = ZNIPPY_E_DST_SMALL; continue; }
        if (len) std::memcpy((uint8_t *)dst + cursor, content[i].data(), (size_t)len);
        cursor += len;
    }
    entry_off[n] = cursor;
    if (status) std::memcpy(status, st.data(), sizeof(int32_t) * n);
    return ZNIPPY_OK;
}

// ---- the content of archived bzip2 and xz files (znippy_archive_bunzip2_files, znippy_archive_unxz_files) -----------------------
// The files are gathered whole on the device (one range read, no copy to the host).  The batch call of the format
// (znippy_bunzip2_batch, znippy_unxz_batch) runs twice there: in measure mode, which gives every file's room (bzip2 names no size
// anywhere; an xz file names it in its indexes), then into those rooms.  Only the contents come back to the host.
// batch(src, src_cap, src_off, src_len, n, out, out_cap, out_room, out_len, status) is that call on the archive's context.
typedef std::function<int(const void *, uint64_t, const uint64_t *, const uint64_t *, uint64_t, void *, uint64_t, const uint64_t *, uint64_t *, int32_t *)> MeasuredBatch;
static int archive_measured_files_impl(znippy_archive *a, const char *const *paths, uint64_t n_files, void *dst, size_t cap, uint64_t *entry_off,
                                       int32_t *status, const char *what, const MeasuredBatch &batch) {
    if (!a || !entry_off || (n_files && !paths) || (cap && !dst)) return fail(ZNIPPY_E_INVAL, "null argument");
    const size_t n = (size_t)n_files;
    const bool sizes_only = !dst && !cap;  // the sizes of the contents alone: entry_off as if every clean file had been written
    std::vector<int32_t> st(n, 0);
    std::vector<FileRange> req;
    std::vector<size_t> who;
    std::vector<uint64_t> fsize(n, 0), measured(n, 0);
    const IndexView view = a->ix.view();
    for (size_t i = 0; i < n; i++) {
        auto it = paths[i] ? a->files.find(paths[i]) : a->files.end();
        if (it == a->files.end()) { st[i] = ZNIPPY_E_INVAL; continue; }
        for (uint64_t r : it->second) fsize[i] += view.row_len(r);
        if (fsize[i] >= (1ull << 32)) { st[i] = ZNIPPY_E_UNSUPPORTED; continue; }
        who.push_back(i);
        req.push_back(FileRange{&it->second, 0, fsize[i]});
    }
    int rc = archive_ctx(a);
    if (rc) return rc;
    std::vector<std::vector<uint8_t>> content(n);
    if (!who.empty()) {
        std::vector<uint64_t> at;
        std::vector<int32_t> rst;
        uint64_t total = 0;
        if ((rc = read_file_ranges(a, req, nullptr, &at, &rst, &total))) return rc;
        ReadBufs &bufs = a->bufs;
        std::vector<size_t> todo;  // indexes into who
        std::vector<uint64_t> s_off, s_len;
        for (size_t k = 0; k < who.size(); k++) {
            if (rst[k]) { st[who[k]] = rst[k]; continue; }
            todo.push_back(k);
            s_off.push_back(at[k]); s_len.push_back(fsize[who[k]]);
        }
        std::vector<uint64_t> o_room(todo.size(), 0), o_len(todo.size(), 0);
        std::vector<int32_t> ist(todo.size(), 0);
        uint64_t out_total = 0;
        if (!todo.empty()) {
            rc = batch(bufs.d_out.p, total, s_off.data(), s_len.data(), todo.size(), nullptr, 0, nullptr, o_room.data(), ist.data());
            if (rc) return fail(rc, std::string(what) + " (measure) failed: " + znippy_last_error(a->ctx));
            for (size_t j = 0; j < todo.size(); j++) {
                if (ist[j] != 0) { st[who[todo[j]]] = ist[j]; o_room[j] = 0; }  // (this status stands; the file takes no room in the second call)
                if (o_room[j] >= (1ull << 32)) { st[who[todo[j]]] = ZNIPPY_E_UNSUPPORTED; o_room[j] = 0; }
                out_total += o_room[j];
            }
            if (sizes_only) {
                for (size_t j = 0; j < todo.size(); j++) measured[who[todo[j]]] = o_room[j];
                todo.clear();
            }
        }
        if (!todo.empty()) {
            if (!bufs.d_blobs.reserve(out_total + 64)) return fail(ZNIPPY_E_NOMEM, "device allocation failed");  // (the chunks in it have been gathered from)
            rc = batch(bufs.d_out.p, total, s_off.data(), s_len.data(), todo.size(), bufs.d_blobs.p, out_total, o_room.data(), o_len.data(), ist.data());
            if (rc) return fail(rc, std::string(what) + " failed: " + znippy_last_error(a->ctx));
            if (!bufs.blob_pin.reserve(out_total + 64)) return fail(ZNIPPY_E_NOMEM, "page-locked allocation failed");
            if (out_total && hipMemcpy(bufs.blob_pin.p, bufs.d_blobs.p, out_total, hipMemcpyDeviceToHost) != hipSuccess) return fail(ZNIPPY_E_HIP, "D2H failed");
            uint64_t o = 0;
            for (size_t j = 0; j < todo.size(); j++) {
                const size_t i = who[todo[j]];
                if (st[i] == 0) st[i] = ist[j];
                if (st[i] == 0) content[i].assign(bufs.blob_pin.p + o, bufs.blob_pin.p + o + o_len[j]);
                o += o_room[j];
            }
        }
    }
    // the contents, packed in file order; one that does not fit is left out and the ones behind it may still fit
    uint64_t cursor = 0;
    for (size_t i = 0; i < n; i++) {
        entry_off[i] = cursor;
        if (st[i]) continue;
        if (sizes_only) { cursor += measured[i]; continue; }
        const uint64_t len = content[i].size();
        if (len > cap - cursor) { st[i] = ZNIPPY_E_DST_SMALL; continue; }
        if (len) std::memcpy((uint8_t *)dst + cursor, content[i].data(), (size_t)len);
        cursor += len;
    }
    entry_off[n] = cursor;
    if (status) std::memcpy(status, st.data(), sizeof(int32_t) * n);
    return ZNIPPY_OK;
}

// ---- the members of archived tars (znippy_archive_list_tar_members) ------------------------------
// The files are gathered whole on the device (one range read, no copy to the host); the first three and the last four bytes of each
// come back (copies queued together, one wait) and say which way it goes and, for a gzip file, its room: gzip files go through
// znippy_gunzip_batch (rooms from ISIZE, the retry rule of znippy_archive_gunzip_files), bzip2 files through znippy_bunzip2_batch
// and xz files through znippy_unxz_batch (both measured, then decoded), the others are copied as they are — all into one device region, the tars, over which one
// znippy_tar_list_batch runs; where every file is a plain tar the listing runs on the gathered files themselves.  Member tables and
// names come back, and the contents when dst is given.
static int znippy_archive_list_tar_members_impl(znippy_archive *a, const char *const *paths, uint64_t n_files, const char *name_prefix, const char *name_suffix,
                                                znippy_tar_member *members, uint64_t members_cap, char *names, uint64_t names_cap, void *dst, size_t cap,
                                                uint64_t *member_first, uint64_t *names_bytes, uint64_t *out_bytes, int32_t *status) {
    if (!a || !member_first || !names_bytes || !out_bytes || (n_files && !paths) || (members_cap && !members) || (names_cap && !names) || (cap && !dst))
        return fail(ZNIPPY_E_INVAL, "null argument");
    const bool measure = !members;
    if (measure && (names || dst)) return fail(ZNIPPY_E_INVAL, "a measuring call takes no buffers");
    const char *prefix = name_prefix ? name_prefix : "", *suffix = name_suffix ? name_suffix : "";
    const size_t n = (size_t)n_files;
    std::vector<int32_t> st(n, 0);
    std::vector<FileRange> req;
    std::vector<size_t> who;
    std::vector<uint64_t> fsize(n, 0);
    const IndexView view = a->ix.view();
    for (size_t i = 0; i <= n; i++) member_first[i] = 0;
    *names_bytes = *out_bytes = 0;
    for (size_t i = 0; i < n; i++) {
        auto it = paths[i] ? a->files.find(paths[i]) : a->files.end();
        if (it == a->files.end()) { st[i] = ZNIPPY_E_INVAL; continue; }
        for (uint64_t r : it->second) fsize[i] += view.row_len(r);
        if (fsize[i] >= (1ull << 32)) { st[i] = ZNIPPY_E_UNSUPPORTED; continue; }
        who.push_back(i);
        req.push_back(FileRange{&it->second, 0, fsize[i]});
    }
    int rc = archive_ctx(a);
    if (rc) return rc;
    enum { PLAIN, GZ, BZ, XZ };
    struct Tar { size_t file; uint64_t src, len; int kind; uint64_t room, off, tar_len; };
    std::vector<Tar> tars;  // in file order
    if (!who.empty()) {
        // the files, whole, on the device
        std::vector<uint64_t> at;
        std::vector<int32_t> rst;
        uint64_t total = 0;
        if ((rc = read_file_ranges(a, req, nullptr, &at, &rst, &total))) return rc;
        ReadBufs &bufs = a->bufs;
        auto most = [&](const Tar &t) { return std::min<uint64_t>(1032 * t.len + 512, 0xFFFFFFF0ull); };
        // 1) which way each file goes, and the rooms of the gzip files: the first three and the last four bytes of every file come
        // to page-locked memory, eight bytes a file, by copies that are all queued before the one wait for them
        if (!bufs.blob_pin.reserve(8 * who.size() + 64)) return fail(ZNIPPY_E_NOMEM, "page-locked allocation failed");
        uint8_t *const ends = bufs.blob_pin.p;
        std::memset(ends, 0, 8 * who.size());
        for (size_t k = 0; k < who.size(); k++) {
            const uint64_t len = fsize[who[k]];
            if (rst[k] || !len) continue;
            const uint8_t *const src = bufs.d_out.p + at[k];
            if (hipMemcpyAsync(ends + 8 * k, src, (size_t)std::min<uint64_t>(len, 3), hipMemcpyDeviceToHost, nullptr) != hipSuccess ||
                (len >= 4 && hipMemcpyAsync(ends + 8 * k + 4, src + len - 4, 4, hipMemcpyDeviceToHost, nullptr) != hipSuccess))
                return fail(ZNIPPY_E_HIP, "D2H failed");
        }
        if (hipStreamSynchronize(nullptr) != hipSuccess) return fail(ZNIPPY_E_HIP, "D2H failed");
        for (size_t k = 0; k < who.size(); k++) {
            if (rst[k]) { st[who[k]] = rst[k]; continue; }
            Tar t{who[k], at[k], fsize[who[k]], PLAIN, 0, 0, 0};
            const uint8_t *const head = ends + 8 * k, *const tail = head + 4;
            if (t.len >= 2 && head[0] == 0x1f && head[1] == 0x8b) t.kind = GZ;
            else if (t.len >= 3 && head[0] == 'B' && head[1] == 'Z' && head[2] == 'h') t.kind = BZ;
            else if (t.len >= 3 && head[0] == 0xFD && head[1] == '7' && head[2] == 'z') t.kind = XZ;
            if (t.kind == GZ && t.len >= 4)
                t.room = std::min<uint64_t>((uint64_t)tail[0] | (uint64_t)tail[1] << 8 | (uint64_t)tail[2] << 16 | (uint64_t)tail[3] << 24, most(t));
            if (t.kind == PLAIN) t.room = t.tar_len = t.len;
            tars.push_back(t);
        }
        // 2) the rooms of the bzip2 and xz files
        std::vector<size_t> bz, xz, gz;
        for (size_t j = 0; j < tars.size(); j++) {
            if (tars[j].kind == BZ) bz.push_back(j);
            else if (tars[j].kind == XZ) xz.push_back(j);
            else if (tars[j].kind == GZ) gz.push_back(j);
        }
        std::vector<uint64_t> s_off, s_len, o_off, o_room, o_len;
        std::vector<int32_t> ist;
        auto lists = [&](const std::vector<size_t> &sel) {
            s_off.clear(); s_len.clear(); o_off.clear(); o_room.clear();
            for (size_t j : sel) { s_off.push_back(tars[j].src); s_len.push_back(tars[j].len); o_off.push_back(tars[j].off); o_room.push_back(tars[j].room); }
            o_len.assign(sel.size(), 0);
            ist.assign(sel.size(), 0);
        };
        // the batch call of a kind over the lists: measure mode without `out`
        auto measured_batch = [&](int kind, size_t n_sel, uint8_t *out, uint64_t out_cap) {
            const uint64_t *off = out ? o_off.data() : nullptr, *room = out ? o_room.data() : nullptr;
            return kind == BZ ? znippy_bunzip2_batch(a->ctx, bufs.d_out.p, total, s_off.data(), s_len.data(), n_sel, out, out_cap, off, room, 0, o_len.data(),
                                                     ist.data(), nullptr, nullptr)
                              : znippy_unxz_batch(a->ctx, bufs.d_out.p, total, s_off.data(), s_len.data(), n_sel, out, out_cap, off, room, o_len.data(), ist.data(),
                                                  nullptr, nullptr, nullptr);
        };
        for (int kind : {BZ, XZ}) {
            const std::vector<size_t> &of_kind = kind == BZ ? bz : xz;
            if (of_kind.empty()) continue;
            lists(of_kind);
            rc = measured_batch(kind, of_kind.size(), nullptr, 0);
            if (rc) return fail(rc, std::string(kind == BZ ? "bunzip2" : "unxz") + " (measure) failed: " + znippy_last_error(a->ctx));
            for (size_t q = 0; q < of_kind.size(); q++) {
                Tar &t = tars[of_kind[q]];
                if (ist[q]) st[t.file] = ist[q];
                else if (o_len[q] >= (1ull << 32)) st[t.file] = ZNIPPY_E_UNSUPPORTED;
                else t.room = o_len[q];
            }
        }
        // 3) the region of the tars: every file's room, on a 16-byte boundary.  With plain tars alone there is nothing to decode and
        // the listing runs where the files were gathered.  Device-to-device copies do not wait on the host and the context's stream
        // is not ordered behind the null stream, so the copies are queued there and waited for before a batch call reads the region.
        DevBuf region;
        uint64_t region_len = 0;
        const bool in_place = bz.empty() && xz.empty() && gz.empty();
        auto give_room = [&](Tar &t) { t.off = region_len; region_len = (region_len + t.room + 15) & ~15ull; };
        if (in_place) {
            for (Tar &t : tars) t.off = t.src;
            region_len = total;
        } else {
            for (Tar &t : tars)
                if (st[t.file] == 0) give_room(t);
            if (!region.reserve(region_len + 64)) return fail(ZNIPPY_E_NOMEM, "device allocation failed");
            for (Tar &t : tars)
                if (t.kind == PLAIN && t.len && hipMemcpyAsync(region.p + t.off, bufs.d_out.p + t.src, t.len, hipMemcpyDeviceToDevice, nullptr) != hipSuccess)
                    return fail(ZNIPPY_E_HIP, "D2D failed");
            if (hipStreamSynchronize(nullptr) != hipSuccess) return fail(ZNIPPY_E_HIP, "D2D failed");
        }
        for (int kind : {BZ, XZ}) {
            std::vector<size_t> sel;
            for (size_t j : kind == BZ ? bz : xz)
                if (st[tars[j].file] == 0) sel.push_back(j);
            if (!sel.empty()) {
                lists(sel);
                rc = measured_batch(kind, sel.size(), region.p, region_len);
                if (rc) return fail(rc, std::string(kind == BZ ? "bunzip2" : "unxz") + " failed: " + znippy_last_error(a->ctx));
                for (size_t q = 0; q < sel.size(); q++) { st[tars[sel[q]].file] = ist[q]; tars[sel[q]].tar_len = o_len[q]; }
            }
        }
        while (!gz.empty()) {
            lists(gz);
            rc = znippy_gunzip_batch(a->ctx, bufs.d_out.p, total, s_off.data(), s_len.data(), gz.size(), region.p, region_len, o_off.data(), o_room.data(), 0,
                                     o_len.data(), ist.data(), nullptr, nullptr);
            if (rc) return fail(rc, std::string("gunzip failed: ") + znippy_last_error(a->ctx));
            std::vector<size_t> again;
            for (size_t q = 0; q < gz.size(); q++) {
                Tar &t = tars[gz[q]];
                st[t.file] = ist[q];
                t.tar_len = o_len[q];
                if (ist[q] == ZNIPPY_E_DST_SMALL && t.room < most(t)) {  // several members: ISIZE names only the last
                    st[t.file] = 0;
                    t.room = std::min<uint64_t>(std::max<uint64_t>(8 * t.room, 4096), most(t));
                    again.push_back(gz[q]);
                }
            }
            if (!again.empty()) {  // a larger region with what there is in front, the new rooms behind
                const uint64_t keep = region_len;
                for (size_t j : again) give_room(tars[j]);
                DevBuf larger;
                if (!larger.reserve(region_len + 64)) return fail(ZNIPPY_E_NOMEM, "device allocation failed");
                if (keep && (hipMemcpyAsync(larger.p, region.p, keep, hipMemcpyDeviceToDevice, nullptr) != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess))
                    return fail(ZNIPPY_E_HIP, "D2D failed");
                std::swap(region.p, larger.p);
                std::swap(region.cap, larger.cap);
            }
            gz.swap(again);
        }
        // 4) one listing over all of them
        std::vector<size_t> sel;
        uint64_t bytes = 0;
        for (size_t j = 0; j < tars.size(); j++)
            if (st[tars[j].file] == 0) { sel.push_back(j); bytes += tars[j].tar_len; }
        if (!sel.empty()) {
            std::vector<uint64_t> t_off, t_len, first(sel.size() + 1, 0);
            for (size_t j : sel) { t_off.push_back(tars[j].off); t_len.push_back(tars[j].tar_len); }
            ist.assign(sel.size(), 0);
            const uint64_t out_cap = dst ? std::min<uint64_t>(cap, bytes) : 0;
            if (dst && !bufs.d_blobs.reserve(out_cap + 64)) return fail(ZNIPPY_E_NOMEM, "device allocation failed");  // (the chunks in it have been gathered from)
            rc = znippy_tar_list_batch(a->ctx, in_place ? bufs.d_out.p : region.p, region_len, t_off.data(), t_len.data(), sel.size(), prefix, strlen(prefix), suffix, strlen(suffix), members,
                                       members_cap, names, names_cap, dst ? bufs.d_blobs.p : nullptr, out_cap, first.data(), names_bytes, out_bytes, ist.data());
            if (rc) return fail(rc, std::string("tar listing failed: ") + znippy_last_error(a->ctx));
            if (dst && *out_bytes && hipMemcpy(dst, bufs.d_blobs.p, *out_bytes, hipMemcpyDeviceToHost) != hipSuccess) return fail(ZNIPPY_E_HIP, "D2H failed");
            size_t q = 0;
            for (size_t i = 0; i < n; i++) {  // (sel is in file order)
                member_first[i] = first[q];
                if (q < sel.size() && tars[sel[q]].file == i) st[i] = ist[q++];
            }
            member_first[n] = first[sel.size()];
        }
    }
    if (status) std::memcpy(status, st.data(), sizeof(int32_t) * n);
    return ZNIPPY_OK;
}

extern "C" {

int znippy_archive_list_tar_members(znippy_archive *a, const char *const *relative_paths, uint64_t n_files, const char *name_prefix, const char *name_suffix,
                                    znippy_tar_member *members, uint64_t members_cap, char *names, uint64_t names_cap, void *dst, size_t cap,
                                    uint64_t *member_first, uint64_t *names_bytes, uint64_t *out_bytes, int32_t *status) {
    return guarded([&] {
        return znippy_archive_list_tar_members_impl(a, relative_paths, n_files, name_prefix, name_suffix, members, members_cap, names, names_cap, dst, cap,
                                                    member_first, names_bytes, out_bytes, status);
    });
}

int znippy_archive_bunzip2_files(znippy_archive *a, const char *const *relative_paths, uint64_t n_files, void *dst, size_t cap, uint64_t *entry_off,
                                 int32_t *status) {
    return guarded([&] {
        return archive_measured_files_impl(a, relative_paths, n_files, dst, cap, entry_off, status, "bunzip2",
                                           [&](const void *src, uint64_t src_cap, const uint64_t *s_off, const uint64_t *s_len, uint64_t n, void *out, uint64_t out_cap,
                                               const uint64_t *room, uint64_t *len, int32_t *st) {
                                               return znippy_bunzip2_batch(a->ctx, src, src_cap, s_off, s_len, n, out, out_cap, nullptr, room, 0, len, st, nullptr, nullptr);
                                           });
    });
}

int znippy_archive_unxz_files(znippy_archive *a, const char *const *relative_paths, uint64_t n_files, void *dst, size_t cap, uint64_t *entry_off,
                              int32_t *status) {
    return guarded([&] {
        return archive_measured_files_impl(a, relative_paths, n_files, dst, cap, entry_off, status, "unxz",
                                           [&](const void *src, uint64_t src_cap, const uint64_t *s_off, const uint64_t *s_len, uint64_t n, void *out, uint64_t out_cap,
                                               const uint64_t *room, uint64_t *len, int32_t *st) {
                                               return znippy_unxz_batch(a->ctx, src, src_cap, s_off, s_len, n, out, out_cap, nullptr, room, len, st, nullptr, nullptr, nullptr);
                                           });
    });
}

int znippy_archive_extract_zip_entries(znippy_archive *a, const char *const *relative_paths, uint64_t n_files, const char *name_prefix,
                                       const char *name_suffix, void *dst, size_t cap, uint64_t *entry_off, int32_t *status) {
    return guarded([&] { return znippy_archive_extract_zip_entries_impl(a, relative_paths, n_files, name_prefix, name_suffix, dst, cap, entry_off, status); });
}

int znippy_archive_extract_tar_members(znippy_archive *a, const char *const *relative_paths, uint64_t n_files, const char *name_prefix,
                                       const char *name_suffix, uint64_t scan_cap, void *dst, size_t cap, uint64_t *entry_off, int32_t *status) {
    return guarded([&] { return znippy_archive_extract_tar_members_impl(a, relative_paths, n_files, name_prefix, name_suffix, scan_cap, dst, cap, entry_off, status); });
}

int znippy_archive_gunzip_files(znippy_archive *a, const char *const *relative_paths, uint64_t n_files, void *dst, size_t cap, uint64_t *entry_off,
                                int32_t *status) {
    return guarded([&] { return znippy_archive_gunzip_files_impl(a, relative_paths, n_files, dst, cap, entry_off, status); });
}

int znippy_archive_block_tree_stats(const znippy_archive *a, uint64_t stats[4]) {
    if (!a || !stats) return ZNIPPY_E_INVAL;
    std::memcpy(stats, a->tree_stats, sizeof a->tree_stats);
    return ZNIPPY_OK;
}

void znippy_archive_close(znippy_archive *a) {
    if (!a) return;
    if (a->ctx) znippy_ctx_destroy(a->ctx);
    if (a->fd >= 0) close(a->fd);
    delete a;
}

// ---- index ------------------------------------------------------------------------------------
static int znippy_index_open_impl(const char *path, znippy_index **out) {
    if (!path || !out) return fail(ZNIPPY_E_INVAL, "null argument");
    std::unique_ptr<znippy_index> ix(new znippy_index());
    int rc = load_index(path, ix.get());
    if (rc) return rc;
    *out = ix.release();
    return ZNIPPY_OK;
}
uint64_t znippy_index_rows(const znippy_index *ix) { return ix ? ix->n() : 0; }
uint64_t znippy_index_manifest_len(const znippy_index *ix) { return ix ? ix->manifest.size() : 0; }
int znippy_index_manifest_entry(const znippy_index *ix, uint64_t i, znippy_manifest_entry *out) {
    if (!ix || !out || i >= ix->manifest.size()) return ZNIPPY_E_INVAL;
    const Manifest &m = ix->manifest[i];
    *out = znippy_manifest_entry{m.pkg_type, m.repo.c_str(), m.module_name.c_str(), m.index_offset, m.index_len, m.row_count};
    return ZNIPPY_OK;
}
int znippy_index_row(const znippy_index *ix, uint64_t i, const char **relative_path, uint32_t *chunk_seq, uint64_t *fdata_offset,
                     int *compressed, uint64_t *uncompressed_size, uint64_t *blob_offset, uint64_t *blob_size,
                     const uint8_t **checksum32) {
    if (!ix || i >= ix->n()) return ZNIPPY_E_INVAL;
    const auto &c = ix->rows.cols;
    if (relative_path) *relative_path = c[0].str[i].c_str();
    if (chunk_seq) *chunk_seq = c[1].u32[i];
    if (fdata_offset) *fdata_offset = c[2].u64[i];
    if (compressed) *compressed = c[3].u8[i];
    if (uncompressed_size) *uncompressed_size = c[4].u64[i];
    if (blob_offset) *blob_offset = c[5].u64[i];
    if (blob_size) *blob_size = c[6].u64[i];
    if (checksum32) *checksum32 = &c[7].u8[32 * i];
    return ZNIPPY_OK;
}
const char *znippy_index_metadata(const znippy_index *ix, const char *key) {
    if (!ix || !key) return nullptr;
    auto it = ix->metadata.find(key);
    return it == ix->metadata.end() ? nullptr : it->second.c_str();
}
void znippy_index_close(znippy_index *ix) { delete ix; }

}  // extern "C"

// ---- the entry points above, behind the exception guard ----
extern "C" {

int znippy_archive_extract_file_verified(znippy_archive *a, const char *relative_path, void *dst, size_t cap, size_t *written) {
    return guarded([&] { return znippy_archive_extract_file_impl(a, relative_path, dst, cap, written, 1); });
}

int znippy_compress_stream(const char *output, int no_skip, int device, znippy_stream **out) {
    return guarded([&] { return znippy_compress_stream_impl(output, no_skip, device, out); });
}

int znippy_stream_send(znippy_stream *s, const char *relative_path, const void *data, size_t len, int pkg_type, const char *repo) {
    return guarded([&] { return znippy_stream_send_impl(s, relative_path, data, len, pkg_type, repo); });
}

int znippy_stream_send_packed(znippy_stream *s, uint64_t n, const char *paths, const uint64_t *path_off, const void *data,
                              const uint64_t *data_off, const int32_t *pkg_type, const char *repo) {
    return guarded([&] { return znippy_stream_send_packed_impl(s, n, paths, path_off, data, data_off, pkg_type, repo); });
}

int znippy_stream_finish(znippy_stream *sp, znippy_compression_report *report) {
    return guarded([&] { return znippy_stream_finish_impl(sp, report); });
}

int znippy_compress_dir(const char *input_dir, const char *output, int no_skip, const char *repo, int device, znippy_compression_report *report) {
    return guarded([&] { return znippy_compress_dir_impl(input_dir, output, no_skip, repo, device, report); });
}

int znippy_decompress_archive(const char *index_path, int save_data, const char *out_dir, int device, uint32_t rank, uint32_t world, znippy_verify_report *report, uint64_t *corrupt_rows, uint64_t corrupt_cap, uint64_t *n_corrupt) {
    return guarded([&] { return znippy_decompress_archive_impl(index_path, save_data, out_dir, device, rank, world, report, corrupt_rows, corrupt_cap, n_corrupt); });
}

int znippy_archive_open(const char *path, int device, znippy_archive **out) {
    return guarded([&] { return znippy_archive_open_impl(path, device, out); });
}

int znippy_archive_extract_file(znippy_archive *a, const char *rel, void *dst, size_t cap, size_t *written) {
    return guarded([&] { return znippy_archive_extract_file_impl(a, rel, dst, cap, written, 0); });
}

int znippy_archive_read_range(znippy_archive *a, const char *rel, uint64_t offset, void *dst, size_t len, size_t *written) {
    return guarded([&] { return znippy_archive_read_range_impl(a, rel, offset, dst, len, written); });
}

int znippy_archive_read_range_verified(znippy_archive *a, const char *rel, uint64_t offset, void *dst, size_t len, size_t *written) {
    return guarded([&] { return znippy_archive_read_range_impl(a, rel, offset, dst, len, written, 1); });
}

int znippy_index_open(const char *path, znippy_index **out) {
    return guarded([&] { return znippy_index_open_impl(path, out); });
}

}  // extern "C"
