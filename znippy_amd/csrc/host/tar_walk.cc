// Host wrappers of the tar walk and the gzip header rule (../tar_rules.h); see tar_walk.h.
#include "tar_walk.h"

#include "../tar_rules.h"

namespace {
constexpr int E_INVAL = -1, E_CORRUPT = -5, E_UNSUPPORTED = -6, E_NOENT = -9;  // the ZNIPPY_E_* of include/znippy_hip.h
int code_of(int verdict) {
    return verdict == tr::TR_FOUND ? 0 : verdict == tr::TR_NOENT ? E_NOENT : verdict == tr::TR_UNSUP ? E_UNSUPPORTED : verdict == tr::TR_MORE ? ZN_TAR_E_MORE : E_CORRUPT;
}
}  // namespace

extern "C" int znippy_tar_find_member(const uint8_t *buf, uint64_t len, int ended, const char *name_prefix, uint64_t prefix_len,
                                      const char *name_suffix, uint64_t suffix_len, uint64_t *data_off, uint64_t *size, uint64_t *need) {
    if ((len && !buf) || (prefix_len && !name_prefix) || (suffix_len && !name_suffix) || !data_off || !size || !need) return E_INVAL;
    *data_off = *size = *need = 0;
    const tr::MemRd rd{buf}, pre{(const uint8_t *)name_prefix}, suf{(const uint8_t *)name_suffix};
    tr::Walk w;
    tr::walk_init(w);
    int v;
    do v = tr::walk_step(w, rd, len, pre, prefix_len, suf, suffix_len);
    while (v == tr::TR_STEP);
    if (v == tr::TR_MORE) {
        if (ended) v = tr::walk_end(w, len);
        else *need = w.need;
    }
    if (v == tr::TR_FOUND) { *data_off = w.data_off; *size = w.size; }
    return code_of(v);
}

extern "C" int znippy_gzip_header(const uint8_t *buf, uint64_t len, uint64_t *deflate_off) {
    if ((len && !buf) || !deflate_off) return E_INVAL;
    *deflate_off = 0;
    const int r = tr::gzip_header(tr::MemRd{buf}, len, deflate_off);
    return r == tr::GZ_SHORT ? ZN_TAR_E_MORE : r;
}
