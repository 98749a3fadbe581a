// The members of tars held in device memory (znippy_tar_list_batch).  A tar walk looks serial — each header says where the next one
// stands — and is done here the way gunzip.hip and bunzip2.hip do their walks: every candidate is judged alone and in parallel, and
// then only the chain from byte 0 counts.  The rules are tar_list_rules.h's, the same text host/tar_list.cc runs serially; the lists
// are host/tar_list_plan.h's.  A node is a 512-byte block of an item, or the end node behind its last whole block.
//
//   tar_scan    one workgroup per chunk of 256 nodes, a half-wave per block: 32 lanes load 16 bytes each (512 contiguous bytes, any
//               alignment; the two halves of a wave read neighbouring blocks), and the zero test, the byte sum and the count of
//               high bytes are reduced over the half-wave (v_sad_u8 sums four bytes an instruction; the checksum field is parsed
//               from the registers of the lane that holds it).  Only a block whose checksum holds is looked at further, by one lane
//               with judge_header — for an 'L' / 'x' / 'X' header with its payload.  Every node gets a record: the node it leads
//               to, its kind, its size.  Terminals (the first of two zero blocks, no header, unsupported, a step past the item's end,
//               the end node) lead to themselves.  A zero block reads the block behind it as well, to know whether it is the first
//               of two.  So the data blocks, nearly all of a tar, are read once; a header (on the chain or not) is read again, with
//               byte loads, by the one lane that judges it, with up to 8 KiB of pax payload, and the headers on the chain once more
//               each by look_back and by the write launch.  Where every second block is a header that lane bounds the scan
//               (DESIGN.md has the figures).
//   tar_chain   rounds of pointer doubling over all nodes of all items: a marked node marks the node its jump pointer names, and
//               the jump pointers square (from one array into the other, so that a round reads only the round before).  After r
//               rounds the nodes up to 2^r - 1 steps from node 0 of their item are marked; the host launches the rounds that close
//               the longest item (tl_rounds), whatever the tars hold.  A mark only ever lands on a node of the chain, so a mark that
//               is seen a round early changes nothing.  No thread walks a chain.
//   tar_emit    pred: every marked node tells its successor who it is.  judge: a marked node that is no extended header looks
//               back over the extended headers directly in front of it ('L', 'x', 'X', 'g', 'K': a run that ends at the first
//               other node) for the name and size they hand on — the earliest of each wins; a zero block or the end with something
//               pending, a size= that differs from the size field, and the extended header that makes a run longer than
//               EXT_RUN_MAX (so that no look back is longer) fail.  The first failing node in stream order gives the
//               item's status (a 64-bit minimum over node << 8 | code; the terminal the chain reaches is its last candidate).
//               Regular members that pass the filter are counted per chunk; prefix: one workgroup turns the chunk sums into
//               prefix sums and item totals; write (after the host has given out room, tl_place): every member writes its record
//               and its name at its place.
//   tar_gather  range_gather.hip, over the pieces the host cuts from the records it has checked (tl_accept).
// Every array is written in full before it is read (nodes, marks and jump pointers by the scan, the second jump array by the first
// round, pick and src by judge, the sums by judge and prefix), the keys are reset by a memset, and pred is read only at marked nodes
// behind the first, each of which has been written by its one predecessor on the chain: DESIGN.md §3a.
#include "common.h"
#include "tar_list_rules.h"

namespace zn {

namespace {

struct RegRd {  // eight bytes a lane holds
    uint64_t f;
    __device__ uint32_t u8(uint64_t off) const { return (uint32_t)(f >> (8 * (off & 7))) & 255; }
};

__device__ __forceinline__ uint32_t half_wave_sum(uint32_t v) {
    for (int m = 16; m; m >>= 1) v += __shfl_xor(v, m, 32);
    return v;
}

__device__ __forceinline__ void load16(uint32_t (&w)[4], const uint8_t *p) { __builtin_memcpy(w, p, 16); }

// inclusive sums of a and b over the workgroup's 256 threads
__device__ __forceinline__ void wg_scan2(uint64_t &a, uint64_t &b, uint64_t (*sh)[256]) {
    const uint32_t tid = threadIdx.x;
    sh[0][tid] = a; sh[1][tid] = b;
    __syncthreads();
    for (uint32_t d = 1; d < 256; d <<= 1) {
        const uint64_t x = tid >= d ? sh[0][tid - d] : 0, y = tid >= d ? sh[1][tid - d] : 0;
        __syncthreads();
        sh[0][tid] += x; sh[1][tid] += y;
        __syncthreads();
    }
    a = sh[0][tid]; b = sh[1][tid];
}

}  // namespace

__global__ __launch_bounds__(256) void k_tar_scan(const TlItem *items, const TlChunk *chunks, TlNode *nodes, uint8_t *mark, uint32_t *jump) {
    const TlChunk ch = chunks[blockIdx.x];
    const TlItem it = items[ch.item];
    const uint32_t tid = threadIdx.x, lane = tid & 31, hw = tid >> 5, half_bit = tid & 32;
    for (uint32_t k = 0; k < ch.n; k += 8) {  // (uniform over the workgroup: the ballots and shuffles below see every lane)
        const uint32_t local = ch.first + k + hw;
        const bool live = k + hw < ch.n, is_block = live && local < it.blocks;
        const uint8_t *const p = it.base + (uint64_t)local * 512 + 16 * lane;
        uint32_t w[4] = {0, 0, 0, 0};
        if (is_block) load16(w, p);
        const bool zero = (uint32_t)(__ballot((w[0] | w[1] | w[2] | w[3]) != 0) >> half_bit) == 0;
        // the checksum field, bytes 148..155, is in lane 9 (bytes 144..159): read as a number, and as eight blanks in the sums
        const RegRd held{w[1] | (uint64_t)w[2] << 32};
        const int64_t mine = tr::number_field(held, 0, 8);
        const int64_t want = (int64_t)((uint64_t)__shfl((uint32_t)mine, 9, 32) | (uint64_t)__shfl((uint32_t)((uint64_t)mine >> 32), 9, 32) << 32);
        if (lane == 9) w[1] = w[2] = 0x20202020u;
        uint32_t sums = 0;  // the byte sum (below 2^20) | the bytes with their top bit set << 20
        for (int q = 0; q < 4; q++) sums += __builtin_amdgcn_sad_u8(w[q], 0, 0) + (__builtin_popcount(w[q] & 0x80808080u) << 20);
        sums = half_wave_sum(sums);
        const int64_t us = sums & 0xFFFFF, high = sums >> 20;
        const bool sum_ok = want == us || want == us - 256 * high;  // (tr::checksum_ok)
        // a zero block: is the one behind it zero too
        const bool look = is_block && zero && local + 1 < it.blocks;
        uint32_t w2[4] = {0, 0, 0, 0};
        if (look) load16(w2, p + 512);
        const bool zero2 = look && (uint32_t)(__ballot((w2[0] | w2[1] | w2[2] | w2[3]) != 0) >> half_bit) == 0;
        if (live && lane == 0) {
            const uint32_t g = it.first_node + local;
            TlNode nd{g, 0, 0};
            if (!is_block) nd.kind = tr::end_kind(it.len);
            else if (zero) {
                nd.kind = zero2 ? tr::K_ZEROS : tr::K_ZERO;
                if (!zero2) nd.succ = g + 1;  // (a block, or the end node)
            } else if (!sum_ok) nd.kind = tr::K_BAD;
            else {
                tr::Block b;
                tr::judge_header(tr::MemRd{it.base}, (uint64_t)local * 512, it.len, b);
                nd.kind = b.kind | (b.type & 255) << 8;
                nd.size = b.size;
                if (!tr::kind_is_terminal(b.kind)) nd.succ = it.first_node + (uint32_t)(b.next / 512);  // (next <= len: a block or the end node)
            }
            nodes[g] = nd;
            jump[g] = nd.succ;
            mark[g] = local == 0;
        }
    }
}

// mark[] is read and written by plain byte loads and stores of threads of one launch, without order between them.  The result does
// not depend on the interleaving: (a) the only value ever stored is 1, and only into mark[jump_in[g]] of a node g that is marked;
// the first node of an item is on its chain, and jump_in[g] is succ applied 2^r times to g, so by induction every mark lands on a
// node of the chain and never on one off it; (b) a thread that sees a mark stored earlier in the same round only marks a further
// node of the chain, a round early; (c) the marks that the rounds are counted on — the nodes up to 2^r - 1 steps from node 0 after
// round r — come from marks of earlier launches, which the stream orders; (d) the host launches tl_rounds(largest item) rounds, the
// bound for a chain through every node, so at the end every node of every chain is marked whatever was seen early, and no other.
// jump_in is only read and jump_out only written in a launch (two arrays), so the pointers have no such race at all.
__global__ __launch_bounds__(256) void k_tar_chain(const uint32_t *jump_in, uint32_t *jump_out, uint8_t *mark, uint32_t n_nodes) {
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    if (g >= n_nodes) return;
    const uint32_t j = jump_in[g];
    if (mark[g]) mark[j] = 1;
    jump_out[g] = jump_in[j];
}

__global__ __launch_bounds__(256) void k_tar_pred(const TlNode *nodes, const uint8_t *mark, uint32_t *pred, uint32_t n_nodes) {
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    if (g >= n_nodes || !mark[g]) return;
    const uint32_t s = nodes[g].succ;
    if (s != g) pred[s] = g;
}

// is node g, an extended header, the one too many of its run: are the EXT_RUN_MAX nodes in front of it extended headers too
__device__ bool run_too_long(const TlItem &it, const TlNode *nodes, const uint32_t *pred, uint32_t g) {
    uint32_t p = g;
    for (uint32_t steps = 0; steps < tr::EXT_RUN_MAX; steps++) {
        if (p == it.first_node) return false;
        const uint32_t q = pred[p];
        if (q >= p || q < it.first_node) return false;  // (cannot happen: a predecessor stands in front, in the same item)
        p = q;
        if (!tr::kind_is_ext(nodes[p].kind & 255)) return false;
    }
    return true;
}

// what the extended headers directly in front of node g hand to it
__device__ void look_back(const TlItem &it, const TlNode *nodes, const uint32_t *pred, uint32_t g, tr::Walk &pend) {
    tr::walk_init(pend);
    const tr::MemRd rd{it.base};
    uint32_t p = g;
    for (uint32_t steps = 0; p != it.first_node && steps < tr::EXT_RUN_MAX; steps++) {  // (a longer run has failed at its header too many)
        const uint32_t q = pred[p];
        if (q >= p || q < it.first_node) break;  // (cannot happen: a predecessor stands in front, in the same item)
        p = q;
        const uint32_t kind = nodes[p].kind & 255;
        if (!tr::kind_is_ext(kind)) break;
        if (kind == tr::K_SKIP) continue;
        tr::Walk w;
        tr::ext_pending(rd, (uint64_t)(p - it.first_node) * 512, kind, nodes[p].size, w);
        if (w.has_name) { pend.has_name = 1; pend.name_off = w.name_off; pend.name_len = w.name_len; }
        if (w.has_size) { pend.has_size = 1; pend.size_over = w.size_over; }
    }
}

__global__ __launch_bounds__(256) void k_tar_emit_judge(const TlItem *items, const TlChunk *chunks, const TlNode *nodes, const uint8_t *mark,
                                                        const uint32_t *pred, const uint8_t *filter, uint32_t prefix_len, uint32_t suffix_len,
                                                        uint32_t *pick, uint32_t *src, TlSum *sums, TlTotal *totals) {
    __shared__ uint64_t sh[2][256];
    const TlChunk ch = chunks[blockIdx.x];
    const TlItem it = items[ch.item];
    const uint32_t tid = threadIdx.x, local = ch.first + tid, g = it.first_node + local;
    const bool live = tid < ch.n;
    uint32_t pk = 0, sr = 0xFFFFFFFFu;
    uint64_t size = 0;
    if (live && mark[g]) {
        const TlNode nd = nodes[g];
        const uint32_t kind = nd.kind & 255;
        uint64_t fail = kind == tr::K_BAD ? TL_KEY_CORRUPT : kind == tr::K_UNSUP ? TL_KEY_UNSUP : 0;
        if (!fail && tr::kind_is_ext(kind)) {
            if (run_too_long(it, nodes, pred, g)) fail = TL_KEY_UNSUP;
        } else if (!fail) {
            tr::Walk pend;
            look_back(it, nodes, pred, g, pend);
            if (kind != tr::K_REG && kind != tr::K_OTHER) {
                if (pend.has_name || pend.has_size) fail = TL_KEY_CORRUPT;  // a name with no member behind it
            } else if (pend.has_size && pend.size_over != nd.size) {
                fail = TL_KEY_UNSUP;
            } else if (kind == tr::K_REG) {
                const tr::MemRd rd{it.base}, pre{filter}, suf{filter + prefix_len};
                const tr::NameOf<tr::MemRd> nm = tr::member_name(rd, (uint64_t)local * 512, pend);
                if (tr::name_matches(nm, pre, prefix_len, suf, suffix_len)) {
                    pk = 0x80000000u | nm.len();
                    size = nd.size;
                    if (pend.has_name) sr = (uint32_t)pend.name_off;
                }
            }
        }
        if (fail) atomicMin((unsigned long long *)&totals[ch.item].key, (unsigned long long)local << 8 | fail);
    }
    if (live) { pick[g] = pk; src[g] = sr; }
    uint64_t a = (uint64_t)(pk >> 31) << 40 | (pk & 0x7FFFFFFFu), b = size;
    wg_scan2(a, b, sh);
    if (tid == 255) sums[blockIdx.x] = TlSum{a >> 40, a & ((1ull << 40) - 1), b};
}

// sums[c] becomes the sum of the chunks in front of c, sums[n_chunks] the sum of all; then the totals of every item
__global__ __launch_bounds__(256) void k_tar_emit_prefix(TlSum *sums, uint32_t n_chunks, const TlItem *items, uint32_t n_items, TlTotal *totals) {
    __shared__ TlSum part[256];
    const uint32_t tid = threadIdx.x, per = (n_chunks + 255) / 256;
    const uint32_t lo = min(tid * per, n_chunks), hi = min(lo + per, n_chunks);
    TlSum s{0, 0, 0};
    for (uint32_t c = lo; c < hi; c++) { s.cnt += sums[c].cnt; s.names += sums[c].names; s.out += sums[c].out; }
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        TlSum run{0, 0, 0};
        for (uint32_t t = 0; t < 256; t++) {
            const TlSum v = part[t];
            part[t] = run;
            run.cnt += v.cnt; run.names += v.names; run.out += v.out;
        }
        sums[n_chunks] = run;
    }
    __syncthreads();
    TlSum run = part[tid];
    for (uint32_t c = lo; c < hi; c++) {
        const TlSum v = sums[c];
        sums[c] = run;
        run.cnt += v.cnt; run.names += v.names; run.out += v.out;
    }
    __threadfence();
    __syncthreads();
    for (uint32_t i = tid; i < n_items; i += 256) {
        const TlSum from = sums[items[i].first_chunk], to = sums[i + 1 < n_items ? items[i + 1].first_chunk : n_chunks];
        totals[i].cnt = to.cnt - from.cnt;
        totals[i].names = to.names - from.names;
        totals[i].out = to.out - from.out;
    }
}

__global__ __launch_bounds__(256) void k_tar_emit_write(const TlItem *items, const TlChunk *chunks, const TlNode *nodes, const uint32_t *pick,
                                                        const uint32_t *src, const TlSum *sums, const TlBase *bases, znippy_tar_member *members,
                                                        uint64_t members_cap, char *names, uint64_t names_cap) {
    __shared__ uint64_t sh[2][256];
    const TlChunk ch = chunks[blockIdx.x];
    const TlBase base = bases[ch.item];
    if (!base.take) return;  // (uniform over the workgroup)
    const TlItem it = items[ch.item];
    const uint32_t tid = threadIdx.x, local = ch.first + tid, g = it.first_node + local;
    const uint32_t pk = tid < ch.n ? pick[g] : 0, nlen = pk & 0x7FFFFFFFu;
    const bool member = pk >> 31;
    const TlNode nd = member ? nodes[g] : TlNode{0, 0, 0};
    uint64_t a = (uint64_t)member << 40 | nlen, b = member ? nd.size : 0;
    wg_scan2(a, b, sh);
    if (!member) return;
    const TlSum here = sums[blockIdx.x], first = sums[it.first_chunk];
    const uint64_t idx = base.member + (here.cnt - first.cnt) + (a >> 40) - 1;
    const uint64_t name_off = base.names + (here.names - first.names) + (a & ((1ull << 40) - 1)) - nlen;
    const uint64_t out_off = base.out + (here.out - first.out) + b - nd.size;
    if (idx >= members_cap || name_off > names_cap || nlen > names_cap - name_off) return;  // (cannot happen: tl_place gave out this room)
    const uint64_t h = (uint64_t)local * 512;
    members[idx] = znippy_tar_member{h, h + 512, nd.size, name_off, out_off, nlen, nd.kind >> 8 & 255};
    const tr::MemRd rd{it.base};
    tr::Walk pend;
    tr::walk_init(pend);
    if (src[g] != 0xFFFFFFFFu) { pend.has_name = 1; pend.name_off = src[g]; pend.name_len = nlen; }
    const tr::NameOf<tr::MemRd> nm = tr::member_name(rd, h, pend);
    for (uint32_t i = 0; i < nlen; i++) names[name_off + i] = (char)nm.at(i);
}

void launch_tar_scan(const TlItem *items, const TlChunk *chunks, uint32_t n_chunks, TlNode *nodes, uint8_t *mark, uint32_t *jump, hipStream_t s) {
    if (n_chunks) hipLaunchKernelGGL(k_tar_scan, dim3(n_chunks), dim3(256), 0, s, items, chunks, nodes, mark, jump);
}
void launch_tar_chain(const uint32_t *jump_in, uint32_t *jump_out, uint8_t *mark, uint32_t n_nodes, hipStream_t s) {
    if (n_nodes) hipLaunchKernelGGL(k_tar_chain, dim3((n_nodes + 255) / 256), dim3(256), 0, s, jump_in, jump_out, mark, n_nodes);
}
void launch_tar_emit(const TlItem *items, uint32_t n_items, const TlChunk *chunks, uint32_t n_chunks, const TlNode *nodes, const uint8_t *mark, uint32_t *pred,
                     uint32_t n_nodes, const uint8_t *filter, uint32_t prefix_len, uint32_t suffix_len, uint32_t *pick, uint32_t *src, TlSum *sums,
                     TlTotal *totals, hipStream_t s) {
    if (!n_chunks) return;
    hipLaunchKernelGGL(k_tar_pred, dim3((n_nodes + 255) / 256), dim3(256), 0, s, nodes, mark, pred, n_nodes);
    hipLaunchKernelGGL(k_tar_emit_judge, dim3(n_chunks), dim3(256), 0, s, items, chunks, nodes, mark, pred, filter, prefix_len, suffix_len, pick, src, sums, totals);
    hipLaunchKernelGGL(k_tar_emit_prefix, dim3(1), dim3(256), 0, s, sums, n_chunks, items, n_items, totals);
}
void launch_tar_emit_write(const TlItem *items, const TlChunk *chunks, uint32_t n_chunks, const TlNode *nodes, const uint32_t *pick, const uint32_t *src,
                           const TlSum *sums, const TlBase *bases, znippy_tar_member *members, uint64_t members_cap, char *names, uint64_t names_cap,
                           hipStream_t s) {
    if (n_chunks) hipLaunchKernelGGL(k_tar_emit_write, dim3(n_chunks), dim3(256), 0, s, items, chunks, nodes, pick, src, sums, bases, members, members_cap, names, names_cap);
}

}  // namespace zn
