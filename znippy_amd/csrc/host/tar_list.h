// The serial listing of a tar for host callers (tar_list.cc): every regular member, by the rules of ../tar_list_rules.h.  Plain C++,
// no HIP call, no I/O, no allocation: a pure function over caller buffers, every read bounds-checked.  It is the CPU oracle of
// znippy_tar_list_batch (tar_list.hip runs the same rules, block by block in parallel) and a helper for bytes already on the host.
#pragma once
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef ZNIPPY_TAR_MEMBER_DEFINED
#define ZNIPPY_TAR_MEMBER_DEFINED
/* one regular member of a tar (znippy_tar_list_batch, znippy_tar_list_members) */
typedef struct {
    uint64_t header_off, data_off, size; /* relative to the tar's first byte: its header, its bytes */
    uint64_t name_off;                   /* its name: name_len bytes at this offset of the names buffer, not terminated */
    uint64_t out_off;                    /* its bytes in the packed output */
    uint32_t name_len, typeflag;         /* typeflag: '0', 0 or '7' */
} znippy_tar_member;
#endif

// Every regular member (typeflag '0', '\0' that is no V7 directory, '7') of the tar buf[0, len), in stream order, whose name starts
// with name_prefix and ends with name_suffix (bytes; either may be empty).  Names are packed into `names`; out_off counts the
// members' sizes up from 0.  members NULL with members_cap 0: nothing is written but the three counts.
//   0                     *n_members, *names_bytes, *out_bytes: what was listed
//   ZNIPPY_E_DST_SMALL    the tar is fine and members_cap or names_cap is not enough: the counts say what is
//   ZNIPPY_E_CORRUPT      a block on the way that is neither zero nor a valid header, a size that is no number, a header, payload or
//                         member that crosses len, a pending name with no member behind it, a bad pax record
//   ZNIPPY_E_UNSUPPORTED  a GNU sparse member, a long-name / pax payload above 8 KiB, len of 4 GiB or more, and the two
//                         deviations of tar_list_rules.h: a pax size= that differs from the member's size field, more than 64
//                         extended headers in a row
//   ZNIPPY_E_INVAL        NULL arguments
// A tar with ZNIPPY_E_CORRUPT or ZNIPPY_E_UNSUPPORTED lists nothing: the counts are 0 (entries of members and names below their
// caps may have been written).
int znippy_tar_list_members(const uint8_t *buf, uint64_t len, const char *name_prefix, uint64_t prefix_len, const char *name_suffix,
                            uint64_t suffix_len, znippy_tar_member *members, uint64_t members_cap, char *names, uint64_t names_cap,
                            uint64_t *n_members, uint64_t *names_bytes, uint64_t *out_bytes);

#ifdef __cplusplus
}
#endif
