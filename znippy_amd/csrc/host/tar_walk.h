// The tar walk and the gzip header rule of ../tar_rules.h for host callers (tar_walk.cc).  Plain C++, no HIP call, no I/O, no
// allocation: pure functions over caller buffers, every read bounds-checked.  The device decoder (targz.hip) runs the same rules.
#pragma once
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

// the answer lies behind the bytes given (ZNIPPY_E_MORE of include/znippy_hip.h)
#define ZN_TAR_E_MORE (-10)

// The first regular member (typeflag '0', '\0' or '7') of the tar whose first `len` bytes are in `buf`, in stream order, whose name
// starts with name_prefix and ends with name_suffix (bytes; either may be empty).  ended: the tar has no byte behind buf[len).
//   0                     *data_off, *size: the member's bytes are buf[*data_off .. + *size), all of them present
//   ZNIPPY_E_NOENT        two zero blocks, or (ended) the tar ends at a header boundary, and no member matched
//   ZNIPPY_E_CORRUPT      a header fails its checksum or its size field is no number, a pax record is malformed, or (ended) the
//                         tar ends inside a header, a long name or the member
//   ZNIPPY_E_UNSUPPORTED  a GNU sparse member, or a long-name / pax payload above 8 KiB, lies in front of the answer
//   ZN_TAR_E_MORE         (not ended) *need: the walk goes on once bytes [0, *need) are there
//   ZNIPPY_E_INVAL        NULL arguments
// data_off, size and need are written on every return but ZNIPPY_E_INVAL (0 where they say nothing).
int znippy_tar_find_member(const uint8_t *buf, uint64_t len, int ended, const char *name_prefix, uint64_t prefix_len, const char *name_suffix,
                           uint64_t suffix_len, uint64_t *data_off, uint64_t *size, uint64_t *need);

// The header of the gzip member (RFC 1952) whose first `len` bytes are in `buf`.
//   0                     *deflate_off: the first byte of the DEFLATE stream (<= len)
//   ZN_TAR_E_MORE         the bytes given end inside the header
//   ZNIPPY_E_CORRUPT      not the magic 1f 8b
//   ZNIPPY_E_UNSUPPORTED  a method other than 8, or a reserved flag bit
// The trailer (CRC-32, ISIZE) is not this function's business, and nothing here checks it.
int znippy_gzip_header(const uint8_t *buf, uint64_t len, uint64_t *deflate_off);

#ifdef __cplusplus
}
#endif
