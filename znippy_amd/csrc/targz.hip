// One member of a gzip-compressed tar (znippy_targz_find_batch): the Cargo.toml of a .crate, the PKG-INFO of an sdist.  A tar has no
// directory: where a member lies is known only while the stream is inflated, and the wanted one usually lies in the first KiB.  So the
// decoder reads the tar as it produces it and stops the moment the answer is known.  wave = stream, as in inflate.hip, and the stream
// decoder is that file's (inflate_dev.h); what is new here is its hook.
//
//   header   the gzip member header (tar_rules.h: gzip_header) is parsed straight from global memory by lane 0, and the bit reader is
//            seated behind it.  The trailer (CRC-32, ISIZE) is never looked at: the call usually stops long before it, and the
//            archive's BLAKE3 is the integrity check of the container.
//   hook     the tar walk (tar_rules.h: walk_step) knows how many bytes of the tar it needs before it can take its next step.  The
//            decoder asks after every symbol that adds bytes whether that many exist (one compare of wave-uniform values); when they
//            do, the gathered literals are flushed, wave_mem_sync makes the wave's own stores readable, and lane 0 steps the walk
//            — in a loop: one match or one stored block may pass several headers — until it wants more bytes or has a verdict.  A
//            header comes at most once per 512 bytes, which cost tens of microseconds to inflate: one lane is enough.
//            The walk's loads go through a reader whose offsets carry a zero the compiler cannot see through, which keeps them
//            vector loads: the scalar cache is not coherent with the stores of this very wave.
//   control  the rules of inflate.hip.  The verdict and the new need come out of lane 0 through readfirstlane before they steer the
//            decoder's loops; the walk itself runs lane-masked and contains no wave primitive and no barrier.  Every step of the
//            walk moves its header offset forward or changes its state on the way to doing so, and reads below the bytes produced.
//   bounds   all tar offsets are 64-bit.  A need beyond the item's cap ends the item at once with ZNIPPY_E_DST_SMALL: nothing is
//            inflated up to the cap first.  A match or stored block that crosses the cap is written up to it and shown to the walk.
// Multi-member gzip files are not guessed at: when the stream ends in front of the answer and another member follows its trailer, the
// item is ZNIPPY_E_UNSUPPORTED.
#include "inflate_dev.h"
#include "tar_rules.h"

namespace zn {

namespace {

constexpr int E_NOENT = -9, E_MORE = -10;  // ZNIPPY_E_NOENT, ZNIPPY_E_MORE

// bytes of the tar in the item's scratch, as vector loads (z: zero, in a VGPR)
struct ScratchRd {
    const uint8_t *p;
    uint32_t z;
    __device__ __forceinline__ uint32_t u8(uint64_t off) const { return p[off + z]; }
    __device__ __forceinline__ uint64_t u64(uint64_t off) const {
        uint64_t v;
        __builtin_memcpy(&v, p + off + z, 8);
        return v;
    }
};

struct TarHook {
    static constexpr bool active = true;
    tr::Walk w;       // lane 0's is the walk; the other lanes' copies are never stepped
    uint64_t need;    // w.need of lane 0 (wave-uniform), at most cap while there is no verdict
    uint32_t cap;
    int verdict;      // 0: none yet; tr::TR_* ; -1: the need lies beyond the cap
    const uint8_t *filter;
    uint32_t prefix_len, suffix_len;

    __device__ __forceinline__ bool due(uint32_t pos) const { return pos >= need; }
    __device__ uint32_t run(const uint8_t *dst, uint32_t pos, uint32_t lane) {
        uint32_t z;
        asm volatile("v_mov_b32 %0, 0" : "=v"(z));
        int v = tr::TR_MORE;
        if (lane == 0) {
            const ScratchRd rd{dst, z};
            const tr::MemRd pre{filter}, suf{filter + prefix_len};
            do v = tr::walk_step(w, rd, pos, pre, prefix_len, suf, suffix_len);
            while (v == tr::TR_STEP);
        }
        v = (int)uni((uint32_t)v);
        need = uni64(w.need);
        if (v != tr::TR_MORE) verdict = v;
        else if (need > cap) verdict = -1;
        return verdict != 0;
    }
};

}  // namespace

__global__ __launch_bounds__(64) void k_targz_find(const TargzItem *items, uint32_t n_items, const uint8_t *filter, uint32_t prefix_len, uint32_t suffix_len,
                                                   TargzResult *res) {
    __shared__ InflLds S;
    const uint32_t lane = threadIdx.x;
    for (uint32_t it = blockIdx.x; it < n_items; it += gridDim.x) {
        __syncthreads();
        const uint8_t *const src = (const uint8_t *)(const glb8 *)uni64((uint64_t)items[it].src);
        uint8_t *const scratch = (uint8_t *)(glb8 *)uni64((uint64_t)items[it].scratch);
        const uint32_t src_len = uni(items[it].src_len), cap = uni(items[it].cap), whole = uni(items[it].whole);
        const int short_input = whole ? E_CORRUPT : E_MORE;  // the input given ends first
        uint64_t at = 0;
        int g = 0;
        if (lane == 0) g = tr::gzip_header(tr::MemRd{src}, src_len, &at);
        g = (int)uni((uint32_t)g);
        at = uni64(at);
        int status;
        uint64_t m_off = 0, m_len = 0;
        uint32_t pos = 0;
        if (g == tr::GZ_SHORT) {
            status = short_input;
        } else if (g != tr::GZ_OK) {
            status = g;
        } else if (cap < tr::BLOCK) {
            status = E_DST;
        } else {
            BitIn b;
            b.src = src + at; b.win = S.in; b.n = src_len - at; b.ip = 0; b.bb = 0; b.bc = 0; b.wbase = 0;
            TarHook hook;
            tr::walk_init(hook.w);
            hook.need = tr::BLOCK; hook.cap = cap; hook.verdict = 0;
            hook.filter = filter; hook.prefix_len = prefix_len; hook.suffix_len = suffix_len;
            const int st = inflate_body(S, b, scratch, cap, lane, hook, &pos);
            if (hook.verdict) {
                const int v = hook.verdict;
                status = v == tr::TR_FOUND ? 0 : v == tr::TR_NOENT ? E_NOENT : v == tr::TR_UNSUP ? E_UNSUP : v == -1 ? E_DST : E_CORRUPT;
                if (v == tr::TR_FOUND) { m_off = uni64(hook.w.data_off); m_len = uni64(hook.w.size); }
            } else if (st == E_INPUT_END) {
                status = short_input;
            } else if (st != 0) {
                status = st;
            } else {
                // the final block ended in front of the answer.  Behind it: what is left of its last byte, the 8-byte trailer, and
                // then nothing — or another member, whose tar bytes would go on where these stopped
                const uint64_t end = b.ip - (b.bc >> 3), tail = b.n - end;
                uint32_t another = 0;
                if (tail >= 18) another = uni((uint32_t)(b.src[end + 8] == 0x1f && b.src[end + 9] == 0x8b));
                if (another) status = E_UNSUP;
                else if (!whole && tail < 18) status = E_MORE;  // whether another member follows lies behind the bytes given
                else status = (int)uni((uint32_t)tr::walk_end(hook.w, pos)) == tr::TR_NOENT ? E_NOENT : E_CORRUPT;
            }
        }
        if (lane == 0) {
            TargzResult r;
            r.status = status; r.pad = 0; r.off = m_off; r.len = m_len; r.scanned = pos;
            res[it] = r;
        }
    }
}

void launch_targz_find(const TargzItem *items, uint32_t n_items, const uint8_t *filter, uint32_t prefix_len, uint32_t suffix_len, TargzResult *res,
                       hipStream_t s) {
    if (n_items)
        hipLaunchKernelGGL(k_targz_find, dim3(n_items < 65536u ? n_items : 65536u), dim3(64), 0, s, items, n_items, filter, prefix_len, suffix_len, res);
}

}  // namespace zn
