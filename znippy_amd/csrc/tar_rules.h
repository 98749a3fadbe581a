// The rules of a gzip member header (RFC 1952) and of a tar stream (USTAR, GNU and PAX as Python's `tarfile` writes and reads them),
// each stated once: where the DEFLATE bytes of a gzip member start, what one 512-byte tar header says (zero block, checksum, size,
// how many data bytes follow its typeflag, its name), and the walk from header to header to the first regular member whose name
// starts with one byte string and ends with another.  The device decoder (targz.hip) runs the walk on the bytes it has inflated so
// far; host/tar_walk.cc wraps it for host callers.  The arbiter is `tarfile` (tests/test_tar_rules_cpu.py runs every function under
// ASan and UBSan against it); where `tarfile` is lenient about damage (a bad later header ends its archive silently, int(s, 8)
// takes signs and underscores) the walk answers with an error code.
// Plain C++: no HIP builtin, no include of the HIP runtime — the qualifiers sit behind ZN_HD, which is empty for a host compiler.
// Bytes come in through a reader object (u8(off), u64(off): the byte / the 8 bytes at offset `off` of the tar); no function reads
// at or behind the `have` (or n) it is given.
//
// Rules that are easy to miss, all `tarfile`'s:
//   - for the link, directory and device types ('1'..'6') no data follows the header, whatever the size field says; every other
//     type, known or not, is followed by its size rounded up to 512
//   - a '\0' member whose 100-byte name field ends with '/' is a directory (old V7 archives)
//   - the prefix field is joined in front of the name ("prefix/name") whenever it is not empty and the type is not a GNU type
//   - a GNU 'L' entry and the path= record of a pax 'x' (or Solaris 'X') entry name the next member; of several in front of one
//     member the first one wins; a pax size= record replaces the member's size field.  'g' and 'K' entries are stepped over (a
//     path= in a global header, which `tarfile` would give to every later member, with them)
//   - the checksum may be the unsigned or the signed byte sum; a size field is octal text or, with 0x80 in front, base 256
// Not followed: GNU sparse members ('S', or GNU.sparse.* pax records), 'L' / 'x' payloads above 8 KiB: TR_UNSUP.
#pragma once
#include <stdint.h>

#ifndef ZN_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define ZN_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define ZN_HD inline
#endif
#endif

namespace tr {

// ---- readers ------------------------------------------------------------------------------------------------------------
struct MemRd {  // plain memory
    const uint8_t *p;
    ZN_HD uint32_t u8(uint64_t off) const { return p[off]; }
    ZN_HD uint64_t u64(uint64_t off) const {
        uint64_t v;
        __builtin_memcpy(&v, p + off, 8);
        return v;
    }
};

// ---- gzip member header -------------------------------------------------------------------------------------------------
// results: GZ_OK (*data_off = the first DEFLATE byte, <= n), GZ_SHORT (the n bytes end inside the header), or a negative code
constexpr int GZ_OK = 0, GZ_SHORT = 1;
constexpr int E_CORRUPT = -5, E_UNSUP = -6;  // ZNIPPY_E_CORRUPT, ZNIPPY_E_UNSUPPORTED

template <class Rd>
ZN_HD int gzip_header(const Rd &rd, uint64_t n, uint64_t *data_off) {
    // magic and method are judged as far as they are there: two bytes that are not 1f 8b are no gzip member however short the input
    if (n >= 1 && rd.u8(0) != 0x1f) return E_CORRUPT;
    if (n >= 2 && rd.u8(1) != 0x8b) return E_CORRUPT;
    if (n >= 3 && rd.u8(2) != 8) return E_UNSUP;
    if (n >= 4 && (rd.u8(3) & 0xE0)) return E_UNSUP;
    if (n < 10) return GZ_SHORT;
    const uint32_t flg = rd.u8(3);
    uint64_t at = 10;  // (MTIME, XFL and OS are not looked at)
    if (flg & 4) {  // FEXTRA
        if (n - at < 2) return GZ_SHORT;
        const uint64_t xlen = rd.u8(at) | (uint64_t)rd.u8(at + 1) << 8;
        at += 2;
        if (n - at < xlen) return GZ_SHORT;
        at += xlen;
    }
    for (uint32_t bit = 8; bit <= 16; bit <<= 1) {  // FNAME, FCOMMENT: zero-terminated
        if (flg & bit) {
            uint32_t c = 1;
            while (at < n && c) c = rd.u8(at++);
            if (c) return GZ_SHORT;
        }
    }
    if (flg & 2) {  // FHCRC (not checked)
        if (n - at < 2) return GZ_SHORT;
        at += 2;
    }
    *data_off = at;
    return GZ_OK;
}

// ---- one tar header -----------------------------------------------------------------------------------------------------
constexpr uint64_t BLOCK = 512;
constexpr uint64_t NAME_PAYLOAD_MAX = 8192;  // 'L' and 'x' payloads above this are not followed
constexpr uint64_t SIZE_LIMIT = 1ull << 62;  // sizes and offsets stay below this: their sums cannot wrap

ZN_HD uint64_t round_block(uint64_t v) { return (v + (BLOCK - 1)) & ~(BLOCK - 1); }

// a numeric field of `len` bytes at `off`: octal text (NUL-terminated, blanks around it, empty = 0) or, with 0x80 in front, a base-256
// number.  -1: not a number this walk follows (bad text, negative, SIZE_LIMIT or more)
template <class Rd>
ZN_HD int64_t number_field(const Rd &rd, uint64_t off, uint32_t len) {
    const uint32_t b0 = rd.u8(off);
    if (b0 == 0x80) {
        uint64_t v = 0;
        for (uint32_t i = 1; i < len; i++) {
            if (v >> 54) return -1;
            v = v << 8 | rd.u8(off + i);
        }
        return v < SIZE_LIMIT ? (int64_t)v : -1;
    }
    if (b0 == 0xFF) return -1;  // negative
    uint32_t n = 0;
    while (n < len && rd.u8(off + n)) n++;
    uint32_t a = 0;
    // str.strip() of Python: blank, \t \n \v \f \r and the four separators 0x1c..0x1f
    while (a < n) { const uint32_t c = rd.u8(off + a); if (c == ' ' || (c >= 9 && c <= 13) || (c >= 0x1c && c <= 0x1f)) a++; else break; }
    while (n > a) { const uint32_t c = rd.u8(off + n - 1); if (c == ' ' || (c >= 9 && c <= 13) || (c >= 0x1c && c <= 0x1f)) n--; else break; }
    uint64_t v = 0;
    for (uint32_t i = a; i < n; i++) {
        const uint32_t c = rd.u8(off + i);
        if (c < '0' || c > '7') return -1;
        v = v << 3 | (c - '0');  // (at most 12 digits: 36 bits)
    }
    return (int64_t)v;
}

template <class Rd>
ZN_HD bool zero_block(const Rd &rd, uint64_t h) {
    uint64_t acc = 0;
    for (uint32_t i = 0; i < BLOCK; i += 8) acc |= rd.u64(h + i);
    return acc == 0;
}

// the checksum field against both sums of the other 504 bytes with the field read as eight blanks
template <class Rd>
ZN_HD bool checksum_ok(const Rd &rd, uint64_t h) {
    uint32_t us = 0, neg = 0;  // the unsigned sum; how many bytes have their top bit set
    for (uint32_t i = 0; i < BLOCK; i += 8) {
        uint64_t v = rd.u64(h + i);
        if (i == 144) v = (v & 0xFFFFFFFFull) | 0x2020202000000000ull;  // bytes 148..151
        if (i == 152) v = (v & ~0xFFFFFFFFull) | 0x20202020ull;          // bytes 152..155
        for (uint32_t k = 0; k < 8; k++) {
            const uint32_t b = (uint32_t)(v >> (8 * k)) & 255;
            us += b;
            neg += b >> 7;
        }
    }
    const int64_t want = number_field(rd, h + 148, 8);
    return want == (int64_t)us || want == (int64_t)us - 256 * (int64_t)neg;
}

// ---- the walk -----------------------------------------------------------------------------------------------------------
// verdicts of walk_step
constexpr int TR_STEP = 0,   // the state advanced: call again
    TR_FOUND = 1,            // w.data_off, w.size: the member, all of it inside [0, have)
    TR_NOENT = 2,            // two zero blocks
    TR_CORRUPT = 3, TR_UNSUP = 4,
    TR_MORE = 5;             // not yet: bytes [0, w.need) have to exist first
enum { W_HEADER = 0, W_PAYLOAD = 1, W_MEMBER = 2 };

struct Walk {
    uint64_t hdr_off;   // where the next header starts
    uint64_t need;      // the next step reads bytes below this
    uint32_t state;
    uint32_t zeros;     // zero blocks in a row
    uint32_t pay_type;  // W_PAYLOAD: the entry whose payload [hdr_off + 512, need) is awaited
    uint32_t has_name, has_size;  // a name / a size for the next member is pending
    uint32_t name_len;
    uint64_t name_off;  // the pending name is bytes [name_off, name_off + name_len) of the tar
    uint64_t size_over;
    uint64_t data_off, size;  // W_MEMBER
};

ZN_HD void walk_init(Walk &w) {
    w.hdr_off = 0; w.need = BLOCK; w.state = W_HEADER; w.zeros = 0; w.pay_type = 0; w.has_name = w.has_size = 0; w.name_len = 0;
    w.name_off = 0; w.size_over = 0; w.data_off = 0; w.size = 0;
}

// the name of the member at header h as a sequence of bytes: the pending name, or prefix "/" name, or name
template <class Rd>
struct NameOf {
    const Rd &rd;
    uint64_t a_off, b_off;  // first part (pending name or prefix), second part (name field)
    uint32_t a_len, b_len, joined;
    ZN_HD uint32_t len() const { return a_len + (joined ? 1 + b_len : 0); }
    ZN_HD uint32_t at(uint32_t i) const { return i < a_len ? rd.u8(a_off + i) : (i == a_len ? (uint32_t)'/' : rd.u8(b_off + (i - a_len - 1))); }
};

template <class Rd>
ZN_HD uint32_t field_len(const Rd &rd, uint64_t off, uint32_t cap) {
    uint32_t n = 0;
    while (n < cap && rd.u8(off + n)) n++;
    return n;
}

template <class Rd, class Fl>
ZN_HD bool name_matches(const NameOf<Rd> &nm, const Fl &pre, uint64_t pre_len, const Fl &suf, uint64_t suf_len) {
    const uint32_t n = nm.len();
    if (pre_len > n || suf_len > n) return false;
    bool ok = true;
    for (uint32_t i = 0; i < (uint32_t)pre_len && ok; i++) ok = nm.at(i) == pre.u8(i);
    for (uint32_t i = 0; i < (uint32_t)suf_len && ok; i++) ok = nm.at(n - (uint32_t)suf_len + i) == suf.u8(i);
    return ok;
}

// the records "<len> <key>=<value>\n" of a pax payload [p, p + n): path= (the last one counts) and size=
template <class Rd>
ZN_HD int pax_records(const Rd &rd, uint64_t p, uint64_t n, Walk &w) {
    uint64_t pos = 0, path_off = 0, size_v = 0;
    uint32_t path_len = 0, got_path = 0, got_size = 0;
    while (pos < n) {
        uint64_t len = 0, i = pos;
        while (i < n && i - pos < 10 && rd.u8(p + i) >= '0' && rd.u8(p + i) <= '9') len = len * 10 + (rd.u8(p + i++) - '0');
        if (i == pos || i >= n || rd.u8(p + i) != ' ') return TR_CORRUPT;
        const uint64_t key = i + 1;
        if (len > n - pos || pos + len < key + 2 || rd.u8(p + pos + len - 1) != '\n') return TR_CORRUPT;
        const uint64_t end = pos + len - 1;  // the newline
        uint64_t eq = key;
        while (eq < end && rd.u8(p + eq) != '=') eq++;
        if (eq == end || eq == key) return TR_CORRUPT;
        const uint64_t kl = eq - key, val = eq + 1;
        const char k_path[] = "path", k_size[] = "size", k_sparse[] = "GNU.sparse.";
        bool is_path = kl == 4, is_size = kl == 4, is_sparse = kl >= 11;
        for (uint32_t k = 0; k < 4 && kl == 4; k++) {
            is_path = is_path && rd.u8(p + key + k) == (uint8_t)k_path[k];
            is_size = is_size && rd.u8(p + key + k) == (uint8_t)k_size[k];
        }
        for (uint32_t k = 0; k < 11 && is_sparse; k++) is_sparse = rd.u8(p + key + k) == (uint8_t)k_sparse[k];
        if (is_sparse) return TR_UNSUP;
        if (is_path) { path_off = p + val; path_len = (uint32_t)(end - val); got_path = 1; }
        if (is_size) {
            uint64_t v = 0;
            if (val == end) return TR_CORRUPT;
            for (uint64_t j = val; j < end; j++) {
                const uint32_t c = rd.u8(p + j);
                if (c < '0' || c > '9' || v >= SIZE_LIMIT / 10) return TR_CORRUPT;
                v = v * 10 + (c - '0');
            }
            size_v = v; got_size = 1;
        }
        pos += len;
    }
    if (got_path && !w.has_name) { w.has_name = 1; w.name_off = path_off; w.name_len = path_len; }
    if (got_size && !w.has_size) { w.has_size = 1; w.size_over = size_v; }
    return TR_STEP;
}

// One step of the walk over bytes [0, have) of the tar.  pre / suf: readers over the two filter strings.
template <class Rd, class Fl>
ZN_HD int walk_step(Walk &w, const Rd &rd, uint64_t have, const Fl &pre, uint64_t pre_len, const Fl &suf, uint64_t suf_len) {
    if (have < w.need) return TR_MORE;
    if (w.state == W_MEMBER) return TR_FOUND;
    const uint64_t h = w.hdr_off;
    if (w.state == W_PAYLOAD) {
        const uint64_t p = h + BLOCK, n = w.need - p;
        if (w.pay_type == 'L') {
            if (!w.has_name) { w.has_name = 1; w.name_off = p; w.name_len = field_len(rd, p, (uint32_t)n); }
        } else {
            const int r = pax_records(rd, p, n, w);
            if (r != TR_STEP) return r;
        }
        w.hdr_off = p + round_block(n);
        w.need = w.hdr_off + BLOCK;
        w.state = W_HEADER;
        return TR_STEP;
    }
    if (h >= SIZE_LIMIT) return TR_CORRUPT;
    if (zero_block(rd, h)) {
        if (w.has_name || w.has_size) return TR_CORRUPT;  // a long name with no member behind it
        if (++w.zeros == 2) return TR_NOENT;
        w.hdr_off = h + BLOCK;
        w.need = w.hdr_off + BLOCK;
        return TR_STEP;
    }
    w.zeros = 0;
    if (!checksum_ok(rd, h)) return TR_CORRUPT;
    const int64_t fsize = number_field(rd, h + 124, 12);
    if (fsize < 0) return TR_CORRUPT;
    uint64_t size = (uint64_t)fsize;
    uint32_t type = rd.u8(h + 156);
    const uint32_t nl = field_len(rd, h, 100);
    if (type == 0 && nl && rd.u8(h + nl - 1) == '/') type = '5';
    if (type == 'S') return TR_UNSUP;
    if (type == 'L' || type == 'x' || type == 'X') {
        if (size > NAME_PAYLOAD_MAX) return TR_UNSUP;
        w.state = W_PAYLOAD;
        w.pay_type = type == 'L' ? 'L' : 'x';
        w.need = h + BLOCK + size;
        return TR_STEP;
    }
    if (type == 'g' || type == 'K') {
        w.hdr_off = h + BLOCK + round_block(size);
        w.need = w.hdr_off + BLOCK;
        return TR_STEP;
    }
    if (w.has_size) size = w.size_over;
    const bool candidate = type == '0' || type == 0 || type == '7';
    if (candidate) {
        const uint32_t pl = field_len(rd, h + 345, 155);
        NameOf<Rd> nm{rd, 0, h, 0, nl, 0};
        if (w.has_name) { nm.a_off = w.name_off; nm.a_len = w.name_len; }
        else if (pl) { nm.a_off = h + 345; nm.a_len = pl; nm.joined = 1; }
        else { nm.a_off = h; nm.a_len = nl; }
        if (name_matches(nm, pre, pre_len, suf, suf_len)) {
            w.state = W_MEMBER;
            w.data_off = h + BLOCK;
            w.size = size;
            w.need = w.data_off + size;
            return TR_STEP;
        }
    }
    w.has_name = w.has_size = 0;
    w.hdr_off = h + BLOCK + (type >= '1' && type <= '6' ? 0 : round_block(size));
    w.need = w.hdr_off + BLOCK;
    return TR_STEP;
}

// The tar is known to end at `have`, below w.need: TR_NOENT at a header boundary with nothing pending, TR_CORRUPT inside a
// header, a payload or the member.
ZN_HD int walk_end(const Walk &w, uint64_t have) {
    return w.state == W_HEADER && have == w.hdr_off && !w.has_name && !w.has_size ? TR_NOENT : TR_CORRUPT;
}

}  // namespace tr
