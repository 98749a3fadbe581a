// ZIP directory locator (zip_dir.h; APPNOTE.TXT 4.3.7, 4.3.12, 4.3.16).  Untrusted input throughout: a field is read only
// after its bytes have been checked to lie inside the caller's buffer, and every offset it yields is checked against the file.
#include "zip_dir.h"

#include <string.h>

namespace {
inline uint32_t rd16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
inline uint32_t rd32(const uint8_t *p) { return rd16(p) | rd16(p + 2) << 16; }
constexpr uint32_t SIG_END = 0x06054b50u, SIG_END64_LOC = 0x07064b50u, SIG_CENTRAL = 0x02014b50u, SIG_LOCAL = 0x04034b50u;
constexpr size_t END_LEN = 22, LOC64_LEN = 20, CENTRAL_LEN = 46, LOCAL_LEN = 30;
}  // namespace

extern "C" {

int znippy_zip_end_of_directory(const uint8_t *tail, size_t tail_len, uint64_t file_size, uint64_t *dir_offset, uint64_t *dir_size,
                                uint64_t *n_entries) {
    if (!tail || !dir_offset || !dir_size || !n_entries || tail_len > file_size) return ZNIPPY_E_INVAL;
    if (tail_len < END_LEN) return ZNIPPY_E_CORRUPT;
    // the record whose comment ends exactly where the file ends, looked for from the back: a comment may hold the signature
    const size_t reach = tail_len < ZN_ZIP_TAIL_MAX ? tail_len : ZN_ZIP_TAIL_MAX;
    for (size_t back = END_LEN; back <= reach; back++) {
        const uint8_t *p = tail + (tail_len - back);
        if (rd32(p) != SIG_END || rd16(p + 20) != back - END_LEN) continue;
        const uint64_t at = file_size - back;  // the record's position in the file
        if (back + LOC64_LEN <= tail_len && rd32(p - LOC64_LEN) == SIG_END64_LOC) return ZNIPPY_E_UNSUPPORTED;  // zip64 locator
        const uint32_t disk = rd16(p + 4), dir_disk = rd16(p + 6), here = rd16(p + 8), total = rd16(p + 10);
        const uint32_t size = rd32(p + 12), off = rd32(p + 16);
        if (total == 0xFFFFu || here == 0xFFFFu || size == 0xFFFFFFFFu || off == 0xFFFFFFFFu || disk == 0xFFFFu || dir_disk == 0xFFFFu)
            return ZNIPPY_E_UNSUPPORTED;  // zip64 markers
        if (disk != 0 || dir_disk != 0 || here != total) return ZNIPPY_E_UNSUPPORTED;  // one of several disks
        if ((uint64_t)off > at || (uint64_t)size > at - off) return ZNIPPY_E_CORRUPT;  // the directory lies in front of the record
        if ((uint64_t)total * CENTRAL_LEN > size) return ZNIPPY_E_CORRUPT;
        *dir_offset = off;
        *dir_size = size;
        *n_entries = total;
        return ZNIPPY_OK;
    }
    return ZNIPPY_E_CORRUPT;
}

int znippy_zip_find_entry(const uint8_t *dir, size_t dir_len, uint64_t n_entries, const char *prefix, size_t prefix_len,
                          const char *suffix, size_t suffix_len, znippy_zip_entry *out) {
    if (!out || (dir_len && !dir) || (prefix_len && !prefix) || (suffix_len && !suffix)) return ZNIPPY_E_INVAL;
    size_t q = 0;
    for (uint64_t i = 0; i < n_entries; i++) {
        if (dir_len - q < CENTRAL_LEN) return ZNIPPY_E_CORRUPT;
        const uint8_t *p = dir + q;
        if (rd32(p) != SIG_CENTRAL) return ZNIPPY_E_CORRUPT;
        const size_t name_len = rd16(p + 28), extra_len = rd16(p + 30), comment_len = rd16(p + 32);
        if (dir_len - q - CENTRAL_LEN < name_len + extra_len + comment_len) return ZNIPPY_E_CORRUPT;
        const uint8_t *name = p + CENTRAL_LEN;
        // prefix and suffix may share bytes of the name (byte-wise comparison, either may be empty)
        if (name_len >= prefix_len && name_len >= suffix_len && (!prefix_len || memcmp(name, prefix, prefix_len) == 0) &&
            (!suffix_len || memcmp(name + (name_len - suffix_len), suffix, suffix_len) == 0)) {
            const uint32_t flags = rd16(p + 8), csize = rd32(p + 20), usize = rd32(p + 24), disk = rd16(p + 34), lho = rd32(p + 42);
            if (flags & 1u) return ZNIPPY_E_UNSUPPORTED;  // encrypted
            if (csize == 0xFFFFFFFFu || usize == 0xFFFFFFFFu || lho == 0xFFFFFFFFu || disk == 0xFFFFu) return ZNIPPY_E_UNSUPPORTED;  // zip64
            if (disk != 0) return ZNIPPY_E_UNSUPPORTED;
            out->local_header_offset = lho;
            out->compressed_size = csize;
            out->uncompressed_size = usize;
            out->crc32 = rd32(p + 16);
            out->method = (uint16_t)rd16(p + 10);
            out->flags = (uint16_t)flags;
            out->name_len = (uint32_t)name_len;
            out->dir_pos = (uint32_t)q;
            return ZNIPPY_OK;
        }
        q += CENTRAL_LEN + name_len + extra_len + comment_len;
    }
    return ZNIPPY_E_NOENT;
}

int znippy_zip_local_data_offset(const uint8_t *header, size_t header_len, uint64_t *data_offset) {
    if (!header || !data_offset) return ZNIPPY_E_INVAL;
    if (header_len < LOCAL_LEN || rd32(header) != SIG_LOCAL) return ZNIPPY_E_CORRUPT;
    if (rd16(header + 6) & 1u) return ZNIPPY_E_UNSUPPORTED;  // encrypted
    if (rd32(header + 18) == 0xFFFFFFFFu || rd32(header + 22) == 0xFFFFFFFFu) return ZNIPPY_E_UNSUPPORTED;  // zip64 sizes
    *data_offset = LOCAL_LEN + (uint64_t)rd16(header + 26) + rd16(header + 28);
    return ZNIPPY_OK;
}

}  // extern "C"
