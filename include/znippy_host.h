/*
 * znippy_host.h — compiled host side of the Znippy hot path (C ABI), layered on znippy_hip.h.
 * Mirrors the reference's pipeline entry points for this path; every function cites what it stands for
 * (paths relative to the reference root).  The reference is Rust; with no Rust toolchain in the image the
 * host layer is C++17 (znippy_amd/csrc/host/), callable from Rust through the same `extern "C"` surface.
 *
 *   znippy_compress_stream / znippy_stream_send / znippy_stream_finish
 *        compress_stream(&PathBuf, no_skip) -> StreamCompressor{sender(), finish()}
 *        znippy-compress/src/stream_packer.rs:L58-87, pipeline L127-372 (reader chunking L146-206,
 *        writer L255-284, finalizer L293-346)
 *   znippy_compress_dir            compress_dir(&input_dir, &output, no_skip, plugin = None, repo) -> CompressionReport
 *        znippy-compress/src/slot_packer.rs:L55-209 (walk L63-78, partition L92-101, big pass rounds L265-280,
 *        small pass rounds L499, one sub-index of both passes L141-189)
 *   znippy_decompress_archive      decompress_archive(index_path, save_data, out_dir) -> VerifyReport
 *        znippy-common/src/decompress.rs:L39-222
 *   znippy_archive_*               ZnippyArchive::{open,file_count,contains/file_size,extract_file}
 *        znippy-common/src/archive.rs:L53-168
 *   znippy_index_*                 read_znippy_index / read_znippy_manifest / interpret_footer
 *        znippy-common/src/index.rs:L269-277,L374-468
 */
#ifndef ZNIPPY_HOST_H
#define ZNIPPY_HOST_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {  /* CompressionReport, znippy-common/src/lib.rs:L39-51 */
    uint64_t total_files, compressed_files, uncompressed_files, total_dirs;
    uint64_t total_bytes_in, total_bytes_out, compressed_bytes, uncompressed_bytes, chunks;
    float compression_ratio;
} znippy_compression_report;

typedef struct {  /* VerifyReport, znippy-common/src/index.rs:L490-499 */
    uint64_t total_files, verified_files, corrupt_files;
    uint64_t total_bytes, verified_bytes, corrupt_bytes, chunks;
} znippy_verify_report;

typedef struct {  /* ManifestEntry, index.rs:L248-256 (strings owned by the handle) */
    int8_t pkg_type;
    const char *repo, *module_name;
    uint64_t index_offset, index_len, row_count;
} znippy_manifest_entry;

typedef struct znippy_stream znippy_stream;
typedef struct znippy_archive znippy_archive;
typedef struct znippy_index znippy_index;

/* Text of the last error on the calling thread ("" if none). */
const char *znippy_host_last_error(void);

/* ---- write side ---- */
/* ZNIPPY_HOST_BLOB_ALIGN=<1|2|...|4096> in the environment (read when a pipeline starts, beside ZNIPPY_HOST_SLOT_MB; an
 * invalid value is 1): every blob_offset of the archive znippy_compress_stream / znippy_compress_dir write is a multiple of
 * it — znippy_rounds_set_blob_align on every slot's rounds table, and every slot written at an aligned offset.  The gaps
 * read as zeros, nothing is added behind the last blob, and the read side needs nothing.
 * ZNIPPY_HOST_BLOCK_TREE=1 in the environment (read at the same moment): both pipelines switch znippy_rounds_emit_block_tree on for
 * every slot's rounds table, fetch each slot's block tree after its encode, keep it by row and, when the metadata layer is written,
 * write the sidecar `<output>.znippy.b3t` beside the archive.  The archive's bytes do not depend on it.  Unset or 0: nothing is
 * emitted and no .b3t file is created, touched or removed.
 * The sidecar, little-endian: 8 bytes "ZNPYB3T1"; u32 block log = 17; u32 zero; u64 n_rows — all rows of the archive, in the order
 * znippy_index_* numbers them; u64 n_entries; then the entries, 32 bytes each, concatenated in row order, in the layout
 * znippy_rows_block_tree_layout gives for a table made from the index columns.  The file is exactly 32 + 32 * n_entries bytes.  It
 * has no checksum of its own: the index's checksum column authenticates every row's entries. */
int znippy_compress_stream(const char *output, int no_skip, int device, znippy_stream **out);
/* pkg_type < 0 = None, repo NULL = None (ArchiveEntry, stream_packer.rs:L34-44). Data is copied (once, into
 * page-locked staging); full staging slots are encoded while the caller keeps sending. */
int znippy_stream_send(znippy_stream *s, const char *relative_path, const void *data, size_t len,
                       int pkg_type, const char *repo);
/* The same for n entries in one call (a caller that already holds its entries packed — the reference's reader stage
 * hands StreamCompressor whole batches, stream_packer.rs:L146-206 — or a binding whose per-call cost matters):
 * entry i has the path paths[path_off[i] .. path_off[i+1]) (no terminator) and the bytes data[data_off[i] .. data_off[i+1]);
 * pkg_type may be NULL (= None for all), repo NULL = None for all.  Stops at the first error. */
int znippy_stream_send_packed(znippy_stream *s, uint64_t n, const char *paths, const uint64_t *path_off,
                              const void *data, const uint64_t *data_off, const int32_t *pkg_type, const char *repo);
/* Drains the pipeline, writes the metadata layer of `<output>.znippy`, fills the report and frees the handle. */
int znippy_stream_finish(znippy_stream *s, znippy_compression_report *report);

/* Directory ingest.  repo NULL = None.  Files are read by a few host threads straight into page-locked staging;
 * metadata plugins are outside this path. */
int znippy_compress_dir(const char *input_dir, const char *output, int no_skip, const char *repo, int device,
                        znippy_compression_report *report);

/* ---- read side ---- */
/* rank/world split the row cursor into contiguous ranges balanced by uncompressed bytes (world = 1:
 * everything).  Counters are this rank's share; total_files is global.  corrupt_rows receives the
 * absolute row numbers with a checksum mismatch (ascending).
 * save_data = 0 is the reference's `verify` (index.rs:L550-553): rows are checked by verify-only runs
 * (znippy_verify_rows), no output region exists on the device and a range is cut by its blob bytes plus the
 * scratch of its compressed rows.  ZNIPPY_NO_VERIFY_ONLY=1 in the environment: every row is decoded into a
 * region that is thrown away, as before (A/B); the report and the corrupt rows are the same either way. */
int znippy_decompress_archive(const char *index_path, int save_data, const char *out_dir, int device,
                              uint32_t rank, uint32_t world, znippy_verify_report *report,
                              uint64_t *corrupt_rows, uint64_t corrupt_cap, uint64_t *n_corrupt);

int znippy_archive_open(const char *path, int device, znippy_archive **out);
uint64_t znippy_archive_file_count(const znippy_archive *a);
int64_t znippy_archive_file_size(const znippy_archive *a, const char *relative_path); /* -1: not found */
int znippy_archive_extract_file(znippy_archive *a, const char *relative_path, void *dst, size_t cap,
                                size_t *written);
/* The same with every chunk's BLAKE3 checked against the index's checksum column (the reference's extract_file has
 * no verification, archive.rs:L144-168; SURVEY §8f rank 1 asks for it): ZNIPPY_E_CHECKSUM on a mismatch. */
int znippy_archive_extract_file_verified(znippy_archive *a, const char *relative_path, void *dst, size_t cap,
                                         size_t *written);
/* pread on an archived file: bytes [offset, offset + len) of it land in dst, clamped at the end of the file — *written is
 * what was copied, 0 for an offset at or past the end.  The range is mapped to the chunks it touches by fdata_offset; only
 * their blobs are read from the archive, and of a chunk this library wrote only the 128 KiB blocks the range overlaps are
 * decoded (znippy_rows_read_ranges on the archive's context).  No checksum is looked at, as for extract_file; a chunk
 * that fails to decode gives its ZNIPPY_E_*, an unknown path ZNIPPY_E_INVAL. */
int znippy_archive_read_range(znippy_archive *a, const char *relative_path, uint64_t offset, void *dst, size_t len,
                              size_t *written);
/* The same pread where every byte returned was covered by a BLAKE3 hash that chains to the index's checksum column
 * (znippy_rows_read_ranges_verified): ZNIPPY_E_CHECKSUM when it was not, and then nothing is copied.  The handle keeps a cache,
 * archive row -> block tree (32 bytes per 128 KiB block of a chunk of more than one block).  The first verified read that touches
 * such a chunk builds its entries once — a whole decode of the chunk whose digest must be the index checksum, ZNIPPY_E_CHECKSUM
 * otherwise; every verified read then installs the cached entries of the chunks it touches (authenticated against the checksum
 * again, znippy_rows_set_block_tree) and hashes only the blocks the range overlaps.  Chunks of at most one block are hashed whole.
 * Blobs are read from the archive file on every call, as for znippy_archive_read_range: damage that appears between two reads is
 * caught for the blocks a read touches.
 * With a sidecar (znippy_archive_open reads `<path>.b3t` if it exists; one that is missing, malformed, or whose n_rows or n_entries
 * disagree with the index is ignored and the open succeeds as without it): the first verified touch of such a chunk offers the
 * sidecar's entries to znippy_rows_set_block_tree instead.  Accepted entries go into the cache without any decode; a rejected chunk
 * falls back to the whole-decode build.  A damaged or forged sidecar therefore costs time, never correctness.  One behaviour comes
 * with it: a fresh handle that reads an undamaged block of a chunk damaged elsewhere succeeds, because only the touched blocks are
 * hashed; without a sidecar that first touch decodes the whole chunk and gives ZNIPPY_E_CHECKSUM. */
int znippy_archive_read_range_verified(znippy_archive *a, const char *relative_path, uint64_t offset, void *dst, size_t len,
                                       size_t *written);
/* stats[0] entries loaded from the sidecar at open (0: none in use); [1] chunks whose sidecar entries were accepted; [2] chunks
 * whose sidecar entries were rejected; [3] chunks whose entries were built by a whole decode. */
int znippy_archive_block_tree_stats(const znippy_archive *a, uint64_t stats[4]);
/* ---- ZIP containers inside the archive ---- */
/* ZIP directory locator (csrc/host/zip_dir.cc): pure functions over caller buffers — no I/O, no allocation, every read bounds-checked,
 * so a crafted container is an error code.  Sizes and the CRC-32 come from the central directory, so entries written with a data
 * descriptor (flag bit 3) need nothing more.  Not supported, each ZNIPPY_E_UNSUPPORTED: zip64 (by its locator or by the 0xFFFFFFFF /
 * 0xFFFF markers), archives of several disks, encrypted entries (flag bit 0).  A malformed record is ZNIPPY_E_CORRUPT.
 * The filter — the first entry, in directory order, whose name starts with `prefix` and ends with `suffix`, compared byte-wise, either
 * may be empty — is this library's: ljar, whose decompress_jar_filter the reference calls, is not part of the reference tree and its
 * rule cannot be read there.  The reference's callers apply exactly this test to what ljar returns
 * (znippy-plugin-maven/src/native.rs:L31: the name ends with "pom.xml"). */
typedef struct {
    uint64_t local_header_offset, compressed_size, uncompressed_size; /* from the central directory */
    uint32_t crc32;
    uint16_t method, flags;
    uint32_t name_len;
    uint32_t dir_pos; /* where the entry's record starts inside the directory */
} znippy_zip_entry;
/* tail: the last tail_len = min(file_size, 65557) bytes of the file (the 22-byte end record behind a comment of up to 65,535 bytes;
 * fewer are accepted, and then a longer comment is not found).  The record taken is the last one whose comment ends exactly where the
 * file ends.  Directory offset, size and entry count are checked against the file: the directory lies in front of the record and
 * holds at least 46 bytes per entry. */
int znippy_zip_end_of_directory(const uint8_t *tail, size_t tail_len, uint64_t file_size, uint64_t *dir_offset, uint64_t *dir_size,
                                uint64_t *n_entries);
/* dir: the dir_len bytes of the central directory.  ZNIPPY_E_NOENT when none of the n_entries entries matches; the zip64, disk and
 * encryption checks are made on the matching entry alone. */
int znippy_zip_find_entry(const uint8_t *dir, size_t dir_len, uint64_t n_entries, const char *prefix, size_t prefix_len,
                          const char *suffix, size_t suffix_len, znippy_zip_entry *out);
/* header: the fixed 30 bytes of the entry's local header (at local_header_offset).  *data_offset = 30 + name length + extra length,
 * both from the local header — they may differ from the central copy; the entry's data starts that far behind the header. */
int znippy_zip_local_data_offset(const uint8_t *header, size_t header_len, uint64_t *data_offset);

/* For every archived file of relative_paths (n_files of them; each a ZIP container: a jar, a war, a wheel): the content of its first
 * entry whose name starts with name_prefix and ends with name_suffix (either may be NULL or empty) — what the reference's ingest
 * plugins ask of ljar::decompress_jar_filter per container, on the read side and for all files at once.  No per-file round trip: one
 * range-read pass (znippy_rows_read_ranges over a table of the chunks touched, so containers stored or compressed, in one chunk or
 * several, all work) fetches every file's last 65,557 bytes, a second one the central directories, a third one each chosen entry's
 * local header and compressed bytes; the compressed streams go to the device in one upload, through one znippy_inflate_batch with the
 * directory's CRC-32s, and come back in one copy.
 * Cost: every pass reads from the archive file, uploads and copies back on its own — of a stored chunk only the requested bytes, of a
 * compressed chunk the whole frame in each pass that touches it; the third pass asks for up to 131,100 bytes beyond an entry's data,
 * because the lengths that place the data are the local header's.
 * Contents are packed in dst: file i at [entry_off[i], entry_off[i + 1]) (entry_off: n_files + 1 values), of length 0 when its status is
 * not 0.  status (optional), per file: 0; ZNIPPY_E_INVAL an unknown path; the locator's codes (ZNIPPY_E_NOENT, ZNIPPY_E_CORRUPT,
 * ZNIPPY_E_UNSUPPORTED); the inflate's codes (ZNIPPY_E_CORRUPT, ZNIPPY_E_CHECKSUM, ZNIPPY_E_UNSUPPORTED for a method other than 0 and 8);
 * ZNIPPY_E_DST_SMALL when cap does not hold it (the files in front of it are unaffected); a chunk's decode error.  The call returns
 * ZNIPPY_OK whatever the files report; NULL arguments give ZNIPPY_E_INVAL. */
int znippy_archive_extract_zip_entries(znippy_archive *a, const char *const *relative_paths, uint64_t n_files,
                                       const char *name_prefix, const char *name_suffix, void *dst, size_t cap,
                                       uint64_t *entry_off /* n_files + 1 */, int32_t *status);
/* For every archived file of relative_paths (each a gzip-compressed tar: a .crate, a .tar.gz sdist, a .tgz): the content of its first
 * regular member whose name starts with name_prefix and ends with name_suffix (either may be NULL or empty) — what the reference's
 * cargo plugin does per crate (znippy-common/src/plugins/cargo_native.rs:L46-71), on the read side and for all files at once.
 * Pass 1 gathers bytes [0, min(file size, head)) of every file on the device — one range-read pass whose result is not copied to the
 * host — and runs the znippy_targz_find_batch of include/znippy_hip.h on them there, a file shorter than head as a whole one; pass 2 does
 * the same with the whole file for exactly the files that reported ZNIPPY_E_MORE.  Only the members come back to the host.  head is
 * 64 KiB; ZNIPPY_HOST_TARGZ_HEAD in the environment, read at the call, overrides it.  scan_cap (at least 512): the most inflated bytes
 * one file may take.
 * Results as in znippy_archive_extract_zip_entries: file i at dst[entry_off[i] .. entry_off[i + 1]) (entry_off: n_files + 1 values), of
 * length 0 when its status is not 0.  status (optional), per file: 0; ZNIPPY_E_INVAL an unknown path; ZNIPPY_E_UNSUPPORTED a file of
 * 4 GiB or more; the per-item codes of that call (ZNIPPY_E_NOENT, ZNIPPY_E_CORRUPT — an empty file too —, ZNIPPY_E_UNSUPPORTED,
 * ZNIPPY_E_DST_SMALL for a member not complete within scan_cap); ZNIPPY_E_DST_SMALL when cap does not hold it (the files in front of
 * it are unaffected); a chunk's decode error.  The call returns ZNIPPY_OK whatever the files report; NULL arguments and a scan_cap
 * below 512 give ZNIPPY_E_INVAL. */
int znippy_archive_extract_tar_members(znippy_archive *a, const char *const *relative_paths, uint64_t n_files,
                                       const char *name_prefix, const char *name_suffix, uint64_t scan_cap, void *dst, size_t cap,
                                       uint64_t *entry_off /* n_files + 1 */, int32_t *status);
/* For every archived file of relative_paths (each a gzip file: a .gz log, a .tar.gz sdist, a .crate, a BGZF file): its whole content,
 * all members concatenated — what the reference's host_decompress (codec 1) does per file through lgz::decompress_gz
 * (znippy-common/src/plugins/wasm_loader.rs), on the read side and for all files at once.  Pass 1 reads the last four bytes of every
 * file, the ISIZE of its last member, which is the content's size when the file has one member.  Pass 2 gathers the files whole on the
 * device — one range-read pass whose result is not copied to the host — and runs the znippy_gunzip_batch of include/znippy_hip.h on
 * them there with those rooms: members and flush segments are decoded in parallel, CRC-32 and ISIZE of every member are checked.  The
 * files that report ZNIPPY_E_DST_SMALL (several members) go through that call again with eight times the room (4 KiB at least), until
 * they fit or the room is what DEFLATE can expand the file to (1032 : 1).  Only the contents come back to the host.
 * Results as in znippy_archive_extract_zip_entries: file i at dst[entry_off[i] .. entry_off[i + 1]) (entry_off: n_files + 1 values), of
 * length 0 when its status is not 0.  status (optional), per file: 0; ZNIPPY_E_INVAL an unknown path; ZNIPPY_E_UNSUPPORTED a file of
 * 4 GiB or more; the per-item codes of that call (ZNIPPY_E_CORRUPT — a file that is no gzip file too —, ZNIPPY_E_CHECKSUM,
 * ZNIPPY_E_UNSUPPORTED); ZNIPPY_E_DST_SMALL when cap does not hold it (the files in front of it are unaffected); a chunk's decode
 * error.  An empty file has no member and no content.  The call returns ZNIPPY_OK whatever the files report; NULL arguments give
 * ZNIPPY_E_INVAL. */
int znippy_archive_gunzip_files(znippy_archive *a, const char *const *relative_paths, uint64_t n_files, void *dst, size_t cap,
                                uint64_t *entry_off /* n_files + 1 */, int32_t *status);
/* For every archived file of relative_paths (each a bzip2 file: a .bz2, a .tar.bz2 / .tbz / .tbz2 source tarball or older sdist): its
 * whole content, all streams concatenated — what the reference's host_decompress (codec 2) does per file through lbzip2
 * (znippy-common/src/plugins/wasm_loader.rs:L18-31, L213-221), on the read side and for all files at once.  The files are gathered
 * whole on the device — one range-read pass whose result is not copied to the host.  bzip2 names the content's size nowhere, so the
 * znippy_bunzip2_batch of include/znippy_hip.h runs twice on them there: in measure mode, which gives every file's room, then into
 * those rooms, blocks decoded in parallel, every block CRC and combined CRC checked.  Only the contents come back to the host.
 * Results as in znippy_archive_gunzip_files: file i at dst[entry_off[i] .. entry_off[i + 1]), of length 0 when its status is not 0.
 * status (optional), per file: 0; ZNIPPY_E_INVAL an unknown path; ZNIPPY_E_UNSUPPORTED a file or a content of 4 GiB or more; the
 * per-item codes of that call (ZNIPPY_E_CORRUPT — a file that is no bzip2 file too —, ZNIPPY_E_CHECKSUM, ZNIPPY_E_UNSUPPORTED);
 * ZNIPPY_E_DST_SMALL when cap does not hold it (the files in front of it are unaffected); a chunk's decode error.  An empty file has
 * no stream and no content.  With dst NULL and cap 0 only the measuring call is made: entry_off holds the offsets the clean files
 * would get, so entry_off[n_files] is the cap that holds them all, and no CRC has been looked at.  The call returns ZNIPPY_OK
 * whatever the files report; NULL arguments give ZNIPPY_E_INVAL.  The members of the tar inside a .tar.bz2 are listed and extracted
 * by znippy_archive_list_tar_members below. */
int znippy_archive_bunzip2_files(znippy_archive *a, const char *const *relative_paths, uint64_t n_files, void *dst, size_t cap,
                                 uint64_t *entry_off /* n_files + 1 */, int32_t *status);
/* For every archived file of relative_paths (each an xz file: a .xz, a .tar.xz / .txz source tarball or package): its whole content,
 * all streams concatenated.  The reference has no xz decoder: such files are in its skip lists, stay stored rows, and a user takes
 * them to liblzma on the host.  The files are gathered whole on the device — one range-read pass whose result is not copied to the
 * host — and the znippy_unxz_batch of include/znippy_hip.h runs twice on them there: in measure mode, which reads the sizes the
 * files' indexes claim and gives every file's room, then into those rooms, every block of every file in one launch, CRC32 and CRC64
 * checks verified.  Only the contents come back to the host.
 * Results, statuses, the sizes-only call (dst NULL, cap 0) and the return value exactly as znippy_archive_bunzip2_files, with the
 * per-item codes of that call (ZNIPPY_E_CORRUPT — a file that is no xz file too —, ZNIPPY_E_CHECKSUM, ZNIPPY_E_UNSUPPORTED:
 * BCJ and delta filters, reserved flags).  Blocks whose check is none, SHA-256 or a reserved id are delivered unverified, as the xz
 * tool delivers them.  The members of the tar inside a .tar.xz are listed and extracted by znippy_archive_list_tar_members below. */
int znippy_archive_unxz_files(znippy_archive *a, const char *const *relative_paths, uint64_t n_files, void *dst, size_t cap,
                              uint64_t *entry_off /* n_files + 1 */, int32_t *status);
#ifndef ZNIPPY_TAR_MEMBER_DEFINED
#define ZNIPPY_TAR_MEMBER_DEFINED
/* one regular member of a tar (include/znippy_hip.h: znippy_tar_list_batch) */
typedef struct {
    uint64_t header_off, data_off, size; /* relative to the tar's first byte: its header, its bytes */
    uint64_t name_off;                   /* its name: name_len bytes at this offset of the names buffer, not terminated */
    uint64_t out_off;                    /* its bytes in the packed output */
    uint32_t name_len, typeflag;         /* typeflag: '0', 0 or '7' */
} znippy_tar_member;
#endif
/* For every archived file of relative_paths (a .tar, a .tar.gz / .tgz / .crate, a .tar.bz2 / .tbz2, a .tar.xz / .txz): every regular member of the tar
 * in it whose name starts with name_prefix and ends with name_suffix (either may be NULL or empty) — what the reference's
 * host_archive_open formats 1 and 2 (wasm_loader.rs: tar_gz_list_entries, tar_bz2_list_entries) return through
 * tar_entries_from_bytes and host_archive_list / host_archive_entry then serve, for all files at once.  The files are gathered whole
 * on the device — one range-read pass whose result is not copied to the host; only the first three and the last four bytes of each
 * come back at this point.  Each goes by its first bytes: 1f 8b through
 * znippy_gunzip_batch, with rooms from ISIZE and the retry rule of znippy_archive_gunzip_files; "BZh" through znippy_bunzip2_batch,
 * in measure mode and then for the decode; fd 37 7a ("\3757z", an xz file) through znippy_unxz_batch in the same two steps; anything
 * else is taken as a plain tar.  One znippy_tar_list_batch of include/znippy_hip.h then
 * lists all the tars there.  Only the member tables and the names come back to the host, and the members' contents when dst is given.
 * Results as in that call: the members of file i are members[member_first[i] .. member_first[i + 1]) (member_first: n_files + 1
 * values; offsets relative to the decompressed tar), their names packed in names, their contents packed in dst at out_off;
 * *names_bytes and *out_bytes say how much of names and dst they take.  With members NULL and members_cap 0 (names and dst NULL too)
 * the tars are only measured: member_first, *names_bytes and *out_bytes are what a call with caps that hold everything reports.
 * status (optional), per file: 0; ZNIPPY_E_INVAL an unknown path; ZNIPPY_E_UNSUPPORTED a file or a tar of 4 GiB or more; the
 * decoders' codes (ZNIPPY_E_CORRUPT, ZNIPPY_E_CHECKSUM, ZNIPPY_E_UNSUPPORTED); the codes of znippy_tar_list_batch: ZNIPPY_E_CORRUPT —
 * a file that is no tar too —, ZNIPPY_E_UNSUPPORTED, ZNIPPY_E_DST_SMALL when a cap does not hold the file's members, names or
 * contents: the files in front of it are unaffected and the ones behind it may still fit; a chunk's decode error.  A file with a
 * status lists no member.  The two deviations from `tarfile` are that call's (include/znippy_hip.h).  The call returns ZNIPPY_OK whatever the files report; NULL arguments give ZNIPPY_E_INVAL. */
int znippy_archive_list_tar_members(znippy_archive *a, const char *const *relative_paths, uint64_t n_files, const char *name_prefix,
                                    const char *name_suffix, znippy_tar_member *members, uint64_t members_cap, char *names,
                                    uint64_t names_cap, void *dst, size_t cap, uint64_t *member_first /* n_files + 1 */,
                                    uint64_t *names_bytes, uint64_t *out_bytes, int32_t *status);
void znippy_archive_close(znippy_archive *a);

/* ---- index / container ---- */
int znippy_index_open(const char *path, znippy_index **out);  /* footer -> manifest -> all sub-indexes */
uint64_t znippy_index_rows(const znippy_index *ix);
uint64_t znippy_index_manifest_len(const znippy_index *ix);
int znippy_index_manifest_entry(const znippy_index *ix, uint64_t i, znippy_manifest_entry *out);
/* Column access for row i (pointers stay valid until close). */
int znippy_index_row(const znippy_index *ix, uint64_t i, const char **relative_path, uint32_t *chunk_seq,
                     uint64_t *fdata_offset, int *compressed, uint64_t *uncompressed_size,
                     uint64_t *blob_offset, uint64_t *blob_size, const uint8_t **checksum32);
/* Value of a schema-metadata key of the first sub-index (NULL if absent). */
const char *znippy_index_metadata(const znippy_index *ix, const char *key);
void znippy_index_close(znippy_index *ix);

/* interpret_footer (index.rs:L269-277): returns 1 = multi (v0.7), 0 = single (v0.6); *offset = payload. */
int znippy_interpret_footer(const uint8_t *tail, size_t n, uint64_t *offset);

/* Serialise / parse a manifest stream (write_manifest_bytes / read_manifest_bytes, index.rs:L291-367).
 * write: returns the byte count, copies up to cap bytes into dst. */
size_t znippy_write_manifest_bytes(const znippy_manifest_entry *entries, size_t n, uint8_t *dst, size_t cap);

#ifdef __cplusplus
}
#endif
#endif
