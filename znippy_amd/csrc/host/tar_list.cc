// The serial tar listing for host callers (../tar_list_rules.h); see tar_list.h.
#include "tar_list.h"

#include "../tar_list_rules.h"

namespace {
constexpr int E_INVAL = -1, E_DST_SMALL = -4, E_CORRUPT = -5, E_UNSUPPORTED = -6;  // the ZNIPPY_E_* of include/znippy_hip.h
}

extern "C" int znippy_tar_list_members(const uint8_t *buf, uint64_t len, const char *name_prefix, uint64_t prefix_len, const char *name_suffix,
                                       uint64_t suffix_len, znippy_tar_member *members, uint64_t members_cap, char *names, uint64_t names_cap,
                                       uint64_t *n_members, uint64_t *names_bytes, uint64_t *out_bytes) {
    if ((len && !buf) || (prefix_len && !name_prefix) || (suffix_len && !name_suffix) || (members_cap && !members) || (names_cap && !names) ||
        !n_members || !names_bytes || !out_bytes)
        return E_INVAL;
    *n_members = *names_bytes = *out_bytes = 0;
    if (len >= (1ull << 32)) return E_UNSUPPORTED;
    const bool measure = !members;
    const tr::MemRd rd{buf}, pre{(const uint8_t *)name_prefix}, suf{(const uint8_t *)name_suffix};
    tr::ListWalk lw;
    tr::list_init(lw);
    uint64_t n = 0, nb = 0, ob = 0;
    bool fits = true;
    int v;
    for (;;) {
        uint64_t h = 0;
        tr::Block b;
        tr::Walk pend;
        v = tr::list_step(lw, rd, len, &h, b, pend);
        if (v == tr::TR_STEP) continue;
        if (v != tr::TR_FOUND) break;
        const tr::NameOf<tr::MemRd> nm = tr::member_name(rd, h, pend);
        if (!tr::name_matches(nm, pre, prefix_len, suf, suffix_len)) continue;
        const uint32_t nl = nm.len();
        if (!measure) {
            fits = fits && n < members_cap && nl <= names_cap - (nb < names_cap ? nb : names_cap);
            if (fits) {
                members[n] = znippy_tar_member{h, h + tr::BLOCK, b.size, nb, ob, nl, b.type};
                for (uint32_t i = 0; i < nl; i++) names[nb + i] = (char)nm.at(i);
            }
        }
        n++; nb += nl; ob += b.size;
    }
    if (v != tr::TR_NOENT) return v == tr::TR_UNSUP ? E_UNSUPPORTED : E_CORRUPT;
    *n_members = n; *names_bytes = nb; *out_bytes = ob;
    return fits ? 0 : E_DST_SMALL;
}
