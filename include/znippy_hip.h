/*
 * znippy_hip.h — C ABI of the MI355X-native per-chunk codec + hash path for the Znippy
 * archive format.  Plain pointers and sizes only; no C++/torch/HIP types in signatures
 * (a HIP stream is passed as `void*`).  Integer status codes, no exceptions, caller-
 * allocated outputs.  Thread-safe for concurrent calls on DISTINCT contexts.
 *
 * What each entry point replaces in the reference (paths relative to the reference root):
 *   znippy_compress_bound        zl_compress_bound             znippy-common/src/codec.rs:L32,L45
 *   znippy_compress              CompressCtx::compress_into    znippy-common/src/codec.rs:L43-55
 *   znippy_get_decompressed_size zl_get_decompressed_size      znippy-common/src/codec.rs:L69
 *   znippy_decompress            codec::decompress_into        znippy-common/src/codec.rs:L67-78
 *   znippy_blake3                blake3::hash                  stream_packer.rs:L219, slot_packer.rs:L553,
 *                                                              decompress.rs:L172
 *   znippy_rows_* + znippy_decode_verify_rows
 *                                body of the read worker loop  znippy-common/src/decompress.rs:L135-190
 *                                (+ stats merge L195-221)      over index columns (index.rs:L43-54)
 *   znippy_verify_rows[_async]   the same loop, save_data=false  znippy-common/src/decompress.rs:L186-189 (the write is
 *                                (`verify`)                     skipped), called from index.rs:L550-553
 *   znippy_decode_rows[_async]   ZnippyArchive::extract_file(s)  znippy-common/src/archive.rs:L144-168 (decode, no checksum)
 *   znippy_rounds_* + znippy_encode_hash_rounds
 *                                barrel + writer bodies        znippy-compress/src/stream_packer.rs:L217-284,
 *                                                              znippy-compress/src/slot_packer.rs:L551-609
 *   znippy_hash_rounds           blake3-only / store path      slot_packer.rs:L553-560 (skip branch)
 *   znippy_inflate_batch         ljar::decompress_jar_filter   znippy-plugin-maven/src/native.rs:L28-31,L47 (the inflate of the
 *                                over a batch of containers     entry the filter chose), znippy-plugin-python/src/native.rs:L85-89
 *   znippy_targz_find_batch      parse_deps_from_tarball        znippy-common/src/plugins/cargo_native.rs:L46-71 (gunzip a .crate, walk
 *                                over a batch of tarballs       the tar to the first .../Cargo.toml); sdists: znippy-plugin-python/src/native.rs:L17-21
 *   znippy_gunzip_batch          lgz::decompress_gz             znippy-common/src/plugins/wasm_loader.rs (host_decompress codec 1,
 *                                over a batch of files          tar_gz_list_entries): the gunzip of a whole file
 *   znippy_bunzip2_batch         lbzip2 (host_decompress 2)     znippy-common/src/plugins/wasm_loader.rs:L18-31,L213-221 (codec 2),
 *                                over a batch of files          L410-441 (tar.bz2): the bunzip2 of a whole file
 *   znippy_unxz_batch            nothing: the reference has no   .xz / .tar.xz / .txz are in its skip lists and stay stored rows; its ecosystem
 *                                xz decoder, it skips the files  list (TODO_NOW.md, "Holger ecosystem") names an LZMA-family decoder, lzip
 *
 * Codec wire format: one standard Zstandard frame (RFC 8878) per chunk.  (The reference's
 * OpenZL framing cannot be reproduced or checked offline — see DESIGN.md "Oracle".)
 */
#ifndef ZNIPPY_HIP_H
#define ZNIPPY_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZNIPPY_OK 0
#define ZNIPPY_E_INVAL (-1)       /* bad argument */
#define ZNIPPY_E_HIP (-2)         /* HIP runtime error (znippy_last_error has the text) */
#define ZNIPPY_E_NOMEM (-3)
#define ZNIPPY_E_DST_SMALL (-4)   /* caller buffer too small */
#define ZNIPPY_E_CORRUPT (-5)     /* malformed frame */
#define ZNIPPY_E_UNSUPPORTED (-6) /* dictionary frames, unknown content size */
#define ZNIPPY_E_CHECKSUM (-7)    /* frame content checksum (XXH64) mismatch */
#define ZNIPPY_E_DIGEST (-8)      /* BLAKE3 of the bytes does not match the index checksum or block tree */
#define ZNIPPY_E_NOENT (-9)       /* no entry of the container matches */
#define ZNIPPY_E_MORE (-10)       /* the answer lies behind the bytes given */

typedef struct znippy_ctx znippy_ctx;
typedef struct znippy_rows znippy_rows;     /* read side: a range of index rows, device-resident */
typedef struct znippy_rounds znippy_rounds; /* write side: a batch of Rounds, device-resident */

/* One context per worker/GPU (the analogue of one CompressCtx per thread, codec.rs:L8-28).
 * `hip_stream` may be NULL (the context then owns a non-blocking stream). */
int znippy_ctx_create(int device, void *hip_stream, znippy_ctx **out);
/* Lifetime rule: a table (znippy_rows, znippy_rounds) holds a reference to the context it was created on.
 * znippy_ctx_destroy on a context that still has tables CLOSES it — every later call that takes this context, with or
 * without a table, returns ZNIPPY_E_INVAL and touches nothing — and the context's memory and device resources are
 * released when its last table is destroyed (znippy_rows_destroy / znippy_rounds_destroy are always safe to call, in
 * any order relative to znippy_ctx_destroy).  Without tables it is released at once.  Calling it twice is harmless
 * while tables keep it alive; after the release the pointer is dangling, as with any destroy call. */
void znippy_ctx_destroy(znippy_ctx *ctx);
/* CompressCtx::new(compression_level) (znippy-common/src/codec.rs:L16-28): the effort of every later encode call of
 * this context.  1..22; a new context starts at 19 (CONFIG.compression_level, common_config.rs:L37).  Two tiers:
 * levels 1-3 use the fast block matcher (one probe per position, raw literals beyond 128 symbols, predefined
 * sequence tables), levels 4-22 the higher effort one (4-way buckets, lazy choice, in-block repeat offsets,
 * per-block entropy tables).  Frames of both tiers are plain RFC 8878.  znippy_ctx_level returns the level. */
int znippy_ctx_set_level(znippy_ctx *ctx, int level);
int znippy_ctx_level(const znippy_ctx *ctx);
/* Opt-in cross-block match window of every later encode call of this context (znippy_compress,
 * znippy_encode_hash_rounds[_async]).  0 (the default): every 128 KiB block of a frame is self-contained, and frames
 * of several blocks end with an empty raw block that says so.  17..27: a match reaches up to 2^window_log bytes back,
 * never in front of the first byte of its own round (rounds stay independent frames): the 64 KiB in front of a block
 * through the block matcher, farther back through long-distance matches found by a per-round index.  Such frames
 * are smaller on big rounds, carry no closing empty block and go through the slower foreign-frame read paths.
 * Blocks are still encoded in parallel (repeat offsets start unknown in every block, no table is shared) and frames
 * are plain single-segment RFC 8878, deterministic, and the same whatever else is in the batch.  Only levels 4-22 use
 * the window; at levels 1-3 the value is kept but frames do not change.  Rounds of at most one block are identical
 * with the window on or off.  znippy_compress_bound / znippy_rounds_blob_bound hold as before.  Other values, and a
 * closed context, give ZNIPPY_E_INVAL.  ZNIPPY_WINDOW_LOG in the environment of znippy_ctx_create sets the initial
 * value.  znippy_ctx_window_log returns it. */
int znippy_ctx_set_window_log(znippy_ctx *ctx, int window_log);
int znippy_ctx_window_log(const znippy_ctx *ctx);
const char *znippy_last_error(const znippy_ctx *ctx);
/* Block until everything the context has queued has finished: its stream, and the streams of its own that carry a part of a
 * run beside it (a read run's verify and counters, the write side's hash and result copy). */
int znippy_ctx_sync(znippy_ctx *ctx);

/* ---- (1) bounds ---------------------------------------------------------------------- */
size_t znippy_compress_bound(size_t n);

/* ---- (5) single-chunk synchronous shims, HOST buffers, codec.rs semantics -------------- */
int znippy_get_decompressed_size(const void *frame, size_t n, uint64_t *out_size);
int znippy_decompress(znippy_ctx *ctx, const void *frame, size_t n, void *dst, size_t cap,
                      size_t *written);
int znippy_compress(znippy_ctx *ctx, const void *src, size_t n, void *dst, size_t cap,
                    size_t *written);
int znippy_blake3(znippy_ctx *ctx, const void *src, size_t n, uint8_t out[32]);

/* ---- (3) batch decode + verify over a row range ---------------------------------------- */
/* Counters of the read loop (WorkerStats, decompress.rs:L22-28; VerifyReport is derived from
 * them on the host, decompress.rs:L195-221).  decode_errors = rows whose frame failed to
 * decode: counted in total_chunks and in no byte counter (decompress.rs:L140,L159-162). */
typedef struct {
    uint64_t total_chunks;
    uint64_t total_written_bytes;
    uint64_t verified_bytes;
    uint64_t corrupt_bytes;
    uint64_t corrupt_rows;
    uint64_t decode_errors;
} znippy_verify_counters;

/* Upload rows [row_begin,row_end) of the index columns (HOST pointers, indexed by absolute
 * row number, exactly the Arrow buffers the reference downcasts at decompress.rs:L115-129):
 *   blob_offset, blob_size, uncompressed_size : u64 per row
 *   compressed_bitmap                         : Arrow boolean bitmap, LSB-first (NULL = all compressed)
 *   checksum                                  : 32 bytes per row (NULL = no verification)
 *   out_offset                                : u64 per row, byte position of the row's decoded
 *                                               bytes in the caller's flat output region
 *                                               (stands for (file, fdata_offset), L186-189).
 *                                               NULL = a table that can only be verified
 *                                               (znippy_verify_rows; a decode call on it
 *                                               returns ZNIPPY_E_INVAL)
 * Also builds the work plan (tiles of <=64 BLAKE3 leaves) that drives the kernels' cursor.
 * What may exceed 4 GiB: every byte position and region size of this interface is a 64-bit value; a blob, a frame, a
 * source round and the output of a stored row may lie across a multiple of 4 GiB.  What may not: a table holds fewer than 2^32 - 16 rows or rounds
 * (ZNIPPY_E_INVAL), and the fast paths take single rows and rounds below 4 GiB only — a compressed row of 4 GiB or more
 * is not split into block items and is left to the serial decoder, the batch path refuses frames whose content size
 * does not fit 32 bits, a table with such a size is uploaded as four 64-bit columns instead of two packed size
 * columns, and the cross-block match window is not used for a round of 4 GiB or more. */
int znippy_rows_create(znippy_ctx *ctx, const uint64_t *blob_offset, const uint64_t *blob_size,
                       const uint8_t *compressed_bitmap, const uint64_t *uncompressed_size,
                       const uint64_t *out_offset, const uint8_t *checksum, uint64_t row_begin,
                       uint64_t row_end, znippy_rows **out);
void znippy_rows_destroy(znippy_rows *rows);
/* Declare the size in bytes of the blob region the table will be run against (d_blobs of the calls below).  Every
 * run validates each row on the host, once per distinct (blob_base, blob_cap, out_cap): a row whose blob does not
 * lie inside [blob_base, blob_base + blob_cap), or whose bytes would not fit inside out_cap, is NOT touched by any
 * kernel and reports ZNIPPY_E_CORRUPT / ZNIPPY_E_DST_SMALL in row_status (counted as a decode error) — a crafted
 * or damaged index is an error code, never a device fault.  Without this call only the output side is checked.
 * A stored row (compressed = 0) is its blob: its length is blob_size, as in the reference (decompress.rs:L143-166). */
int znippy_rows_set_blob_cap(znippy_rows *rows, uint64_t blob_cap);

/* Decode-or-passthrough + BLAKE3 + compare for every row of the table.
 *   d_blobs   : DEVICE pointer to the blob region; row r's blob is d_blobs[blob_offset[r]-blob_base ..]
 *   d_out     : DEVICE pointer to the flat output region (row r lands at d_out + out_offset[r]);
 *               out_cap = its size in bytes
 *   counters  : HOST, filled after the call (the call synchronises the stream)
 *   corrupt_rows / corrupt_cap : HOST list receiving absolute row numbers whose checksum
 *               mismatched (ascending); may be NULL
 *   row_status: HOST, optional (NULL ok): one int32 per row of the table, 0 = decoded, <0 = ZNIPPY_E_*
 * Asynchronous variant: znippy_decode_verify_rows_async queues the work only; results are read
 * back with znippy_rows_results after znippy_ctx_sync.
 * Device memory a context takes for this call beyond the table's own columns (kept until the context goes): pools of the
 * batch path sized from the table's content (literals 1 byte, sequence records 1.5, decoding tables 1 per content byte of
 * its compressed rows, each capped at 16 GiB) and — only for tables with compressed rows above 64 KiB — 4 bytes per byte of
 * those rows for the resolve path, capped at 8 GiB (ZNIPPY_NO_RX=1 in the environment of znippy_ctx_create: none, such
 * frames are then executed by one wave each).  A pool that cannot be allocated is not an error: its path is not used.
 * The bytes in d_out belong to the caller once a results call for that run has returned (znippy_rows_results,
 * znippy_rows_results_lagged, znippy_rows_digests — the synchronous call ends in one): a table whose previous run needed
 * nothing behind its main kernel is run without the kernels that stand behind it, and a run that turns out to have needed
 * them after all (the blobs changed) is repeated in full, with the arguments it was given, inside the first results call
 * that looks at it.  A repeat is invisible in the run sequence: znippy_rows_results_lagged still returns each queued run's
 * own counters, once its d_out is complete.  When the repeated run is not the latest one, the latest run is repeated in
 * full after it, so that a flagged run queued behind it is complete as well and the table's status column, corrupt list
 * and digests (znippy_rows_results, znippy_rows_digests) again describe the latest run.  d_blobs / d_out of a queued run
 * must therefore stay valid until its results have been read, and those of the latest run until the run before it has
 * been read as well (ZNIPPY_NO_LEAN=1 in the environment of znippy_ctx_create: every run is a full one).  A failed
 * queueing call that had already queued work leaves the table with no readable run.
 * Ordering: a run's kernels that write d_out are queued on the context's stream, so work queued there behind the call sees
 * the bytes of every row the run decoded.  The run's verify, its counters and the event the results calls wait for may be
 * queued on a stream of the context's own beside the NEXT run's kernels (a table keeps two sets of control block, status
 * column, digests and corrupt list — 44 bytes per row more — and run k uses set k & 1): the context's stream alone does
 * not order them.  Every results call, znippy_ctx_sync and the destroy calls wait for them (ZNIPPY_NO_FORK_VERIFY=1 in the
 * environment of znippy_ctx_create: every run's verify on the context's stream, as before).
 * Run lanes: on a context that owns its stream (znippy_ctx_create with hip_stream == NULL) a run without those kernels may
 * also be queued beside the run queued directly in front of it instead of behind it, on a second stream of the context's own
 * (run k of a table on lane k & 1; lane 0 is the context's stream): its clear executes while the earlier run's kernel runs and
 * its workgroups take over each CU as the earlier run's leave.  Two runs are left unordered only when neither can see the other:
 * both are such runs; they belong to different tables or use the two sets of one table; the bytes they write cannot differ —
 * either is a verify-only run, or [d_out, d_out + out_cap) of the two are disjoint, or table, d_blobs, blob_base, the declared
 * blob size (znippy_rows_set_blob_cap), d_out and out_cap are all identical (the blobs of a queued run may not change, so both
 * write the same bytes); and neither run's blob region overlaps the other's output region (a blob region of undeclared size
 * qualifies in the identical case only).  Otherwise the run waits for the earlier run's kernel, as it always did.  Everything
 * else queued through the context — a full run, another kind of call, a call on another table, the write side — stands behind
 * every such run queued before it, and such a run stands behind everything queued before it on the context's stream.  A context
 * created on a caller's stream never does this: work queued on that stream behind a call sees the run's bytes, literally.
 * ZNIPPY_NO_RUN_LANES=1 (or ZNIPPY_NO_FORK_VERIFY=1) in the environment of znippy_ctx_create: every run in queue order on the
 * context's stream. */
int znippy_decode_verify_rows(znippy_ctx *ctx, znippy_rows *rows, const void *d_blobs,
                              uint64_t blob_base, void *d_out, uint64_t out_cap,
                              znippy_verify_counters *counters, uint64_t *corrupt_rows,
                              uint64_t corrupt_cap, int32_t *row_status);
int znippy_decode_verify_rows_async(znippy_ctx *ctx, znippy_rows *rows, const void *d_blobs,
                                    uint64_t blob_base, void *d_out, uint64_t out_cap);
/* Verify only: the read loop with save_data=false (decompress.rs:L186-189; `verify`, index.rs:L550-553) — every blob is
 * read, decoded as far as hashing it needs, hashed and compared, and no output is written.  It takes the place of a
 * znippy_decode_verify_rows[_async] call whose d_out is thrown away.  The results are read with the same three calls
 * (znippy_rows_results, _results_lagged, znippy_rows_digests) and are what a decode run of the same table over the same
 * blobs reports — total_written_bytes included, which the reference counts whatever save_data is (decompress.rs:L168-169).
 * A verify run is a run like any other in the table's sequence: it takes a slot of the two-run ring, uses and updates what
 * the table remembers of its last run (it may be a lean run, and is then repeated as a verify run if it comes back
 * flagged), and may be queued between decode runs on the same table; it never writes into a d_out an earlier decode run
 * was given.  Rows outside the declared blob region report ZNIPPY_E_CORRUPT as before; there is no output side to check.
 * Rows of the periodic shape the fused kernels recognise, the periodic and raw blocks of big multi-block frames and stored
 * rows are hashed where they are (on chip, or in the blob region).  Only rows that go through a decoder need their bytes
 * in memory: those land in a scratch region the CONTEXT owns — one 16-byte aligned slot per compressed row with bytes,
 * sized by the table's compressed rows (a table without one takes none), grow-only, kept until the context goes, capped at
 * 16 GiB: a table that needs more returns ZNIPPY_E_NOMEM and queues nothing.  Runs of one context are ordered on its stream
 * and the auxiliary streams join before a run ends, so runs in flight — of one table or several — share the region. */
int znippy_verify_rows(znippy_ctx *ctx, znippy_rows *rows, const void *d_blobs, uint64_t blob_base,
                       znippy_verify_counters *counters, uint64_t *corrupt_rows, uint64_t corrupt_cap,
                       int32_t *row_status);
int znippy_verify_rows_async(znippy_ctx *ctx, znippy_rows *rows, const void *d_blobs, uint64_t blob_base);
/* Decode only: the extract path, which never looks at the checksum column (ZnippyArchive::extract_file / extract_files,
 * znippy-common/src/archive.rs:L144-168) — every row is decoded (or, if stored, copied) to d_out + out_offset[r], exactly where and
 * as a decode run places it, and nothing is hashed: no digest is computed and the checksum column, if the table has one, is not read.
 * It takes the place of a znippy_decode_verify_rows[_async] call on a table created with checksum = NULL, without the hash that
 * call still pays for.  Counters, status column and the bytes in d_out are what that call reports for a table built from the same
 * columns with checksum = NULL over the same blobs: verified_bytes == total_written_bytes, corrupt_bytes == corrupt_rows == 0,
 * decode_errors and every row's ZNIPPY_E_* are identical.  The results are read with znippy_rows_results / _results_lagged;
 * znippy_rows_digests returns ZNIPPY_E_INVAL while the latest run of the table is a decode-only run (there are no digests), and
 * works again after the next decode or verify-only run.  A table without out_offset returns ZNIPPY_E_INVAL; the host's validation of
 * every row against the blob region and out_cap is the decode run's.  A decode-only run is a run like any other in the table's
 * sequence: it takes a slot of the two-run ring and may be queued between decode and verify-only runs of the same table with two
 * runs in flight.  It is never a lean run, never comes back flagged, and neither uses up nor updates what the table remembers of
 * its last run; when an earlier flagged run forces the latest run to be repeated, a decode-only run is repeated as one.  It writes
 * only into the d_out it was given.  Every allocation it needs is made before its first stream operation; a failed queueing call
 * that had already queued work leaves the table with no readable run, as for a decode run. */
int znippy_decode_rows(znippy_ctx *ctx, znippy_rows *rows, const void *d_blobs, uint64_t blob_base, void *d_out,
                       uint64_t out_cap, znippy_verify_counters *counters, int32_t *row_status);
int znippy_decode_rows_async(znippy_ctx *ctx, znippy_rows *rows, const void *d_blobs, uint64_t blob_base, void *d_out,
                             uint64_t out_cap);
int znippy_rows_results(znippy_ctx *ctx, znippy_rows *rows, znippy_verify_counters *counters,
                        uint64_t *corrupt_rows, uint64_t corrupt_cap, int32_t *row_status);
/* Counters of the run `lag` (0 or 1) runs before the latest one queued on this table: waits for THAT run only,
 * so a caller that keeps two runs in flight reads run k's counters while run k+1 executes — the read loop
 * reports after the loop, not per row (decompress.rs:L195-221).  ZNIPPY_E_INVAL if no such run exists. */
int znippy_rows_results_lagged(znippy_ctx *ctx, znippy_rows *rows, unsigned lag, znippy_verify_counters *counters);
/* Computed digests of the last run (HOST, 32 bytes per row of the table). */
int znippy_rows_digests(znippy_ctx *ctx, znippy_rows *rows, uint8_t *digests);

/* Byte ranges of rows: what an artifact server answering a range request, or a reader that wants the ZIP central directory of an
 * archived file first and one entry afterwards (TODO_NOW.md:L200-213), asks for — without paying for the whole chunk (a row is up to
 * 10 MiB, common_config.rs:L39).  All range arrays are HOST arrays of n_ranges entries:
 *   range_row    absolute row number of the table
 *   range_begin, range_len   bytes of the row's decoded content (its length is uncompressed_size, blob_size for a stored row)
 *   range_out    where the range lands in d_out; NULL = the ranges are packed back to back in array order (range i at the sum of the
 *                lengths in front of it, whatever their status)
 *   range_status HOST, optional: 0 or ZNIPPY_E_* per range
 *   decoded_bytes HOST, optional: the content bytes the decoders produced in this call — the content size of every block decoded on
 *                its own, plus uncompressed_size of every row decoded whole; nothing for stored rows.  The call's measure of work.
 * Bytes: for every range with status 0 the bytes at its destination are bytes [begin, begin + len) of what a whole-row decode of that
 * row writes, whenever that decode succeeds.  Writes: no byte of d_out outside the destinations of status-0 ranges is written;
 * destinations must not overlap (not checked); len == 0 with begin <= the row's length is status 0 and writes nothing.
 * Partial decode: a compressed row of >= 2 blocks (and below 4 GiB) whose frame passes the block scan — this library's frames with the
 * window off: self-contained 128 KiB blocks — has only the blocks decoded that overlap at least one requested range of the row, each
 * once per call however many ranges touch it and in whatever order, provided each decodes from a clean state.  Such a range reports 0
 * even if a block it never looked at is damaged: the call vouches for what it decoded and for nothing else, as extract_file does
 * without a checksum.  Fallback: anything else — a one-block row, another writer's frame, a window frame, a row of 4 GiB or more, a
 * frame the scan does not accept, a needed block that turns out to need history — is decoded whole into scratch and the range copied
 * out; a row whose whole decode fails gives every range on it the ZNIPPY_E_* that znippy_decode_rows reports for that row.  A range of
 * a stored row is a copy out of the blob region.
 * Host validation, per range, before any kernel runs: row outside the table, or begin + len overflowing or past the row's length:
 * ZNIPPY_E_INVAL; destination not inside out_cap: ZNIPPY_E_DST_SMALL; the row's blob outside the declared blob region
 * (znippy_rows_set_blob_cap): ZNIPPY_E_CORRUPT.  No kernel touches such a range and the call still returns ZNIPPY_OK, as a run does
 * with bad rows.  ZNIPPY_E_INVAL is returned only for NULL arguments, a closed context or a table of another context; n_ranges == 0
 * is ZNIPPY_OK.
 * Not a run: the call is synchronous, ordered on the context's stream behind whatever is queued, takes no slot of the two-run ring and
 * neither reads nor updates what the table remembers of its last run; status column, corrupt list, digests and foreign stats stay as
 * they are.  It works on tables created without out_offset or without checksum, and may be called between an async run and the read
 * of its results without changing what either reports (znippy_last_kernel_times then describes this call: range_scan,
 * range_decode_blocks, range_decode_rows, range_decode_rows_late — the rows a block pass gave up on —, range_copy).
 * Scratch: decoded blocks and fallback rows land in a region the CONTEXT owns — grow-only, kept until the context goes, capped at
 * 16 GiB like the verify scratch.  A call that needs more returns ZNIPPY_E_NOMEM: the blocks and the rows known up front to need a
 * whole decode are sized before anything is queued; rows the block pass gives up on are sized after it, with the stream idle, and
 * a refusal there still comes before the first byte of d_out is written.  Every offset is a 64-bit value. */
int znippy_rows_read_ranges(znippy_ctx *ctx, znippy_rows *rows, const void *d_blobs, uint64_t blob_base,
                            const uint64_t *range_row, const uint64_t *range_begin, const uint64_t *range_len,
                            const uint64_t *range_out, uint64_t n_ranges,
                            void *d_out, uint64_t out_cap, int32_t *range_status, uint64_t *decoded_bytes);

/* ---- block tree: range reads verified block by block against the row checksum ----------------------------------------
 * BLAKE3 is a tree hash and 128 KiB is 128 chunks, a power of two: every aligned 128 KiB block of a row is a complete subtree of the
 * row's hash tree.  With the chaining values of these subtrees a block can be checked on its own, and the chaining values authenticate
 * themselves — folded together they must give the row's `checksum` (the construction BLAKE3 was designed for: Bao).
 * Definitions.  len = a row's content length (uncompressed_size; blob_size for a stored row), BLK = 131072.
 *   A row has nb = (len > BLK && len < 4 GiB) ? ceil(len / BLK) : 0 entries: rows of at most one block, and rows of 4 GiB or more, are
 *   verified whole against `checksum` and need none.
 *   Entry k is the NON-root chaining value of the BLAKE3 subtree over chunks [128k, min(128k + 128, ceil(len / 1024))) of the row's
 *   content: the chunk counters are the row's own (128k + i), the last chunk may be short, the subtree has the usual left-heavy shape
 *   (pairwise folding with the odd node promoted gives it), a last block of one chunk is that chunk's chaining value (CHUNK_START |
 *   CHUNK_END, no parent) and ROOT is never set.  An entry is serialised as eight little-endian 32-bit words (32 bytes).
 *   The row's digest is the same pairwise fold over its nb >= 2 entries with ROOT on the last parent.
 *   The block tree of a table is the entries of its rows, concatenated in row order: 32 bytes per 128 KiB, 0.024 % of the content.
 * Trust.  The tree may come from anywhere — znippy_rows_block_tree_build, a file beside the archive, another machine.  The index
 * checksum alone is the root of trust: znippy_rows_set_block_tree accepts a row's entries only if they fold to the row's checksum, and
 * a block is accepted only if its bytes hash to an accepted entry.  Forging either means a BLAKE3 collision.
 * All four calls are synchronous, ordered on the context's stream, and NOT runs, under the rules of znippy_rows_read_ranges: no slot of
 * the two-run ring; the table's remembered last run, status column, corrupt list and digests are untouched; they may be called
 * between an async run and the read of its results (znippy_last_kernel_times then describes the call).  NULL arguments (other than
 * the optional ones), a closed context or a table of another context give ZNIPPY_E_INVAL.
 *
 * znippy_rows_block_tree_layout: *n_entries = entries of the whole table; row_first (HOST, n + 1 values, optional): row i's entries
 * are [row_first[i], row_first[i + 1]).
 *
 * znippy_rows_block_tree_build computes the tree from the blobs (tree: HOST, 32 * n_entries bytes; may be NULL when n_entries is 0).
 * Rows without entries are not looked at (status 0).  Every other compressed row is decoded whole into context scratch by a private
 * decode-only run — the range scratch, sized before anything is queued; more than its cap gives ZNIPPY_E_NOMEM with nothing queued —
 * stored rows are hashed where they lie in the blob region, one launch produces all entries, and on a table with a checksum column
 * each row's entries are folded and compared with its checksum (a table without one compares nothing).  row_status (HOST, optional,
 * one per row): 0; the decode run's ZNIPPY_E_* for a row that failed to decode; ZNIPPY_E_CORRUPT for a blob outside the declared blob
 * region (host validation, as in a run); ZNIPPY_E_DIGEST for a digest mismatch.  The entries of a row whose status is not 0 are written
 * as zeros.  The call does not install the tree.
 *
 * znippy_rows_set_block_tree installs a tree (HOST, 32 * n_entries bytes; NULL removes the installed one).  Needs a table created
 * with a checksum column (ZNIPPY_E_INVAL otherwise).  The entries are uploaded and every row with entries is authenticated: row_status
 * (optional) is 0 — accepted, or a row without entries — or ZNIPPY_E_DIGEST — rejected.  The call returns ZNIPPY_OK either way: a
 * rejected row is simply a row without entries from then on.  The table keeps a device copy and the per-row verdicts until
 * znippy_rows_destroy; a second call replaces them.
 *
 * znippy_rows_read_ranges_verified: znippy_rows_read_ranges — host validation, destinations, packing, decoded_bytes, scratch rules
 * and fallbacks are exactly that call's — on a table created with a checksum column (ZNIPPY_E_INVAL otherwise), where a range reports
 * 0 only if EVERY BYTE IT RETURNS WAS COVERED BY A HASH THAT CHAINS TO THE ROW'S CHECKSUM.  Routes:
 *   by blocks  a compressed row on the partial route whose entries are accepted: after the block pass each decoded block is hashed
 *              from the scratch and compared with its entry (kernel time: range_verify_blocks);
 *   stored     a stored row whose entries are accepted: the blocks its ranges overlap are hashed in place in the blob region;
 *   whole      a row of at most one block; a row without accepted entries (no tree installed, or the row was rejected — such a
 *              row is not tried block by block); every row the unverified call decodes whole (a foreign or window frame, a frame
 *              the scan refuses, a "late" row, a row of 4 GiB or more): the private table of the whole-row pass gets the rows'
 *              checksums and runs decode + verify instead of decode-only.  A stored row on this route is hashed whole where it
 *              lies by a private verify-only run (kernel time: range_verify_rows).
 * A block or row that fails gives ZNIPPY_E_DIGEST to every range that overlaps it; decode errors keep their codes.  Verification
 * happens before the gather: no byte of a range whose status is not 0 is written.  len == 0 ranges are status 0 and verify nothing.
 * hashed_bytes (HOST, optional): the content bytes hashed in this call, the hash-side twin of decoded_bytes — the content size of
 * every distinct block hashed on its own, each once per call however many ranges touch it, plus the length of every row hashed whole. */
int znippy_rows_block_tree_layout(znippy_ctx *ctx, znippy_rows *rows, uint64_t *n_entries, uint64_t *row_first);
int znippy_rows_block_tree_build(znippy_ctx *ctx, znippy_rows *rows, const void *d_blobs, uint64_t blob_base, uint8_t *tree,
                                 int32_t *row_status);
int znippy_rows_set_block_tree(znippy_ctx *ctx, znippy_rows *rows, const uint8_t *tree, int32_t *row_status);
int znippy_rows_read_ranges_verified(znippy_ctx *ctx, znippy_rows *rows, const void *d_blobs, uint64_t blob_base,
                                     const uint64_t *range_row, const uint64_t *range_begin, const uint64_t *range_len,
                                     const uint64_t *range_out, uint64_t n_ranges, void *d_out, uint64_t out_cap,
                                     int32_t *range_status, uint64_t *decoded_bytes, uint64_t *hashed_bytes);

/* ---- raw DEFLATE of ZIP entries the engine already holds ----------------------------------------------------------------
 * What the ingest plugins do to every jar, war and wheel (ljar::decompress_jar_filter, znippy-plugin-maven/src/native.rs:L28-31, batched
 * at L47; znippy-plugin-python/src/native.rs:L85-89): one small entry of a ZIP container is found through the central directory and only
 * that entry is inflated (TODO_NOW.md:L200-213: the filter comes before any decompression work).  The container bytes are in device
 * memory already — the staging slot on the write side, the blob region or the output of a range read on the read side; this call turns a
 * batch of such entries into their content without leaving the device.  Raw DEFLATE (RFC 1951) only: no gzip, zlib or deflate64 framing.
 * All arrays are HOST arrays of n entries:
 *   src_off, src_len   item i's compressed bytes are d_src[src_off[i] .. + src_len[i]); src_cap = size of the region at d_src
 *   method             ZIP's numbers; NULL = every item is 8.  8: DEFLATE.  0: a copy, which needs src_len == out_len (ZNIPPY_E_CORRUPT
 *                      otherwise).  Anything else: ZNIPPY_E_UNSUPPORTED
 *   out_off            where item i lands in d_out; NULL = the outputs are packed back to back in array order (item i at the sum of the
 *                      out_len in front of it, whatever their status)
 *   out_len            the size the content must have (the central directory has it)
 *   crc32              optional: the ZIP CRC-32 the content must have; a mismatch on an otherwise clean item is ZNIPPY_E_CHECKSUM
 *   status             HOST, optional: 0 or ZNIPPY_E_* per item
 *   crc_out            HOST, optional: the CRC-32 (ZIP polynomial, reflected) of the bytes produced, computed on the device, whenever the
 *                      stream decoded to out_len bytes — status 0, and ZNIPPY_E_CHECKSUM, where it is the computed value; undefined for
 *                      every other status
 * Per item, a stream is valid exactly when zlib's raw inflate accepts it: block type 3, a stored block whose LEN is not the complement of
 * NLEN, HLIT above 286 or HDIST above 30, a repeat without a previous length or past HLIT + HDIST (the two sets of lengths are one
 * sequence: a repeat may cross from one into the other), an over-subscribed set, an incomplete code-length set, an incomplete
 * literal/length or distance set unless its longest code has one bit, a missing symbol 256, decoded symbols 286, 287 or distance symbols
 * 30, 31, a distance beyond the bytes produced so far and input that ends before the final block's end-of-block are ZNIPPY_E_CORRUPT.
 * Every check of a symbol comes before its first output byte.  A symbol that would write past out_len is ZNIPPY_E_DST_SMALL; the final
 * block's end-of-block with fewer than out_len bytes produced is ZNIPPY_E_CORRUPT; bytes of src_len behind the final block are ignored.
 * A damaged stream is a status, never a fault, a hang or a write outside the item's destination.
 * Host validation, per item, before any kernel runs: source not inside [0, src_cap), or off + len overflowing: ZNIPPY_E_INVAL;
 * destination not inside out_cap: ZNIPPY_E_DST_SMALL; src_len or out_len of 4 GiB or more: ZNIPPY_E_UNSUPPORTED; then the method.  No
 * kernel touches such an item and the call still returns ZNIPPY_OK, whatever the items report.  ZNIPPY_E_INVAL is returned only for NULL
 * required arguments (src_off, src_len, out_len; d_src and d_out when n > 0), a closed context, or n of 2^32 - 16 or more; n == 0 is
 * ZNIPPY_OK.
 * Writes: no byte of d_out outside the destinations of the items is written; inside the destination of an item whose status is not 0 the
 * bytes are unspecified; destinations must not overlap (not checked).  Every offset is a 64-bit value.
 * Not a run: the call is synchronous, ordered on the context's stream behind whatever is queued, takes no slot of any table's two-run
 * ring and leaves every table untouched.  It may be called between an async run and the read of its results without changing what that
 * run reports (znippy_last_kernel_times then describes this call: inflate, inflate_crc).  Every allocation is made before the first
 * stream operation.
 * Kernels: one wave decodes one stream, its decoding tables in LDS (csrc/inflate.hip); the CRC is a launch of its own in which a
 * workgroup splits an entry across its 256 lanes and folds the lane CRCs by multiplying with x^(8 len) mod P, as zlib's crc32_combine. */
int znippy_inflate_batch(znippy_ctx *ctx, const void *d_src, uint64_t src_cap, const uint64_t *src_off, const uint64_t *src_len,
                         const uint8_t *method, void *d_out, uint64_t out_cap, const uint64_t *out_off, const uint64_t *out_len,
                         const uint32_t *crc32, uint64_t n, int32_t *status, uint32_t *crc_out);

/* ---- one tar member out of gzip-compressed tars the engine already holds ----------------------------------------------------
 * The third registry type of the reference (znippy-common/src/plugins/cargo_native.rs:L46-71: a .crate is gunzipped and its tar walked to
 * the first .../Cargo.toml; znippy-plugin-python/src/native.rs:L17-21 lists .tar.gz sdists beside wheels).  Such files sit in the archive as
 * stored gzip streams.  A tar has no directory — where a member lies is known only while the stream is inflated — so this call decodes
 * each stream only until the tar it produces answers the question: "the filter happens before any decompression work"
 * (TODO_NOW.md:L200-213) becomes "stop the moment the answer is known".  Plain .tar, xz tarballs and multi-member gzip are out of
 * scope; a bzip2 tarball is decompressed whole by znippy_bunzip2_batch, which finds no member.
 *   d_src, src_cap     DEVICE: the region that holds the files; item i is the gzip member d_src[src_off[i] .. + src_len[i])
 *   whole              HOST, optional (NULL: every item is whole): 0 = item i is only the head of its file
 *   name_prefix/suffix the filter, compared as bytes as in znippy_zip_find_entry: the first regular member (typeflag '0', '\0', '7') in
 *                      stream order whose name starts with the one and ends with the other wins
 *   scan_cap           at least 512: the most inflated bytes one item may take.  Item i gets min(scan_cap, 1032 * src_len + 512) bytes (no
 *                      valid DEFLATE expands more; below 4 GiB - 16 in any case), rounded up to 16, of the context's grow-only range
 *                      scratch, capped at 16 GiB: a batch that needs more returns ZNIPPY_E_NOMEM with nothing queued
 *   d_out, out_cap     DEVICE: the members with status 0 are packed back to back in array order
 *   out_off, out_len   HOST out: where member i lies in d_out; 0, 0 for an item with another status
 *   status             HOST, optional: per item, see below
 *   scanned            HOST, optional: bytes inflated per item
 * Per item: 0; ZNIPPY_E_NOENT — the tar ended (two zero blocks, or the final block ends at a header boundary) and no member matched;
 * ZNIPPY_E_CORRUPT — no gzip magic, a DEFLATE stream zlib's raw inflate refuses, a tar header that fails its checksum or whose size is
 * no number, a final block that ends inside a header or member, input of a whole item that ends first; ZNIPPY_E_MORE — input of an item
 * that is not whole ends first (inside the gzip header, inside the stream, or so closely behind it that a following member could not
 * be seen): ask again with more of the file; ZNIPPY_E_UNSUPPORTED — a method other than 8 or reserved flag bits in the gzip header,
 * a GNU sparse member, a long-name or pax payload above 8 KiB, or 10 or more bytes that start another gzip member behind the 8-byte
 * trailer (multi-member files are not guessed at); ZNIPPY_E_DST_SMALL — the member is not complete within the item's scan bytes (an
 * item ends at once when the walk needs bytes beyond them: nothing is inflated up to the cap first), or it no longer fits into out_cap
 * (it takes no room, and members behind it may still fit).  The rules of the walk, with Python's tarfile as arbiter: csrc/tar_rules.h.
 * The gzip trailer (CRC-32, ISIZE) is never checked: the call usually stops long before it.  The archive's BLAKE3 is the integrity
 * check of the container.
 * Host validation, per item, before any kernel runs: source not inside [0, src_cap), or off + len overflowing: ZNIPPY_E_INVAL; src_len
 * of 4 GiB or more: ZNIPPY_E_UNSUPPORTED.  No kernel touches such an item and the call returns ZNIPPY_OK whatever the items report.
 * ZNIPPY_E_INVAL is returned only for NULL required arguments, a filter string of 64 KiB or more, scan_cap below 512, a closed context
 * or n of 2^32 - 16 or more; n == 0 is ZNIPPY_OK.
 * Writes: no byte of d_out outside the packed members is written.  Not a run, and synchronous on the context's stream, exactly as
 * znippy_inflate_batch; no table is touched; every allocation is made before the first stream operation
 * (znippy_last_kernel_times: targz_find, targz_gather).
 * Kernels: one wave decodes one stream with the decoder of znippy_inflate_batch and steps the tar walk on what it has produced
 * (csrc/targz.hip); the members are moved by the range reads' gather. */
int znippy_targz_find_batch(znippy_ctx *ctx, const void *d_src, uint64_t src_cap, const uint64_t *src_off, const uint64_t *src_len,
                            const uint8_t *whole, uint64_t n, const char *name_prefix, uint64_t prefix_len, const char *name_suffix,
                            uint64_t suffix_len, uint64_t scan_cap, void *d_out, uint64_t out_cap, uint64_t *out_off, uint64_t *out_len,
                            int32_t *status, uint64_t *scanned);

/* ---- whole gzip files the engine already holds ---------------------------------------------------------------------------------
 * The plain gunzip of the reference's ingest side (host_decompress codec 1 and tar_gz_list_entries of wasm_loader.rs, both through
 * lgz::decompress_gz, which splits the stream at full-flush boundaries and decompresses the pieces in parallel): .gz logs, .tar.gz sdists,
 * .crate files, BGZF files, all of which sit in the archive as stored rows.  The DEFLATE decoder of znippy_inflate_batch is one wave per
 * stream; this call cuts a file where it can be cut — gzip members are independent, and behind the empty stored block 00 00 FF FF of a
 * flush point (Z_FULL_FLUSH, Z_SYNC_FLUSH, pigz) symbol decoding needs nothing from before it — and gives every piece a wave.
 *   d_src, src_cap     DEVICE: the region that holds the files; item i is the whole file d_src[src_off[i] .. + src_len[i])
 *   d_out, out_cap     DEVICE: item i's content goes to d_out[out_off[i] .. + out_room[i]), its room
 *   out_off            HOST, optional (NULL: the rooms lie back to back in array order)
 *   out_room           HOST: the bytes item i may produce.  For a file of one member the trailer's ISIZE (its last 4 bytes) is exact
 *   seg_min            the least distance in source bytes between two kept flush candidates of an item (below); 0 = the default,
 *                      256 bytes (the best of the values swept in profiles/gunzip_report.log), which ZNIPPY_GZ_SEG_MIN (a decimal number
 *                      of bytes) replaces for every call
 *   out_len            HOST out: bytes produced; 0 for every status but 0
 *   status             HOST, optional: per item, see below
 *   members            HOST out, optional: gzip members decoded (status 0)
 *   segments           HOST out, optional: the pieces of item i that a wave of its own decoded (status 0; empty pieces count)
 * Per item, with Python's gzip.decompress as arbiter: the content of all members, concatenated.  Zero bytes behind a trailer are
 * ignored; anything else there that is no member header is ZNIPPY_E_CORRUPT; an item of no bytes has no member and no content.  The
 * header rule is that of znippy_targz_find_batch (csrc/tar_rules.h: gzip_header): FEXTRA, FNAME and FCOMMENT are skipped, FHCRC is
 * skipped and not verified, and — the one deviation from the arbiter — a method other than 8 or reserved FLG bits are
 * ZNIPPY_E_UNSUPPORTED.  A DEFLATE stream is valid exactly when zlib's raw inflate accepts it (the rules at znippy_inflate_batch);
 * input that ends early — inside a header, a stream or a trailer — is ZNIPPY_E_CORRUPT.  More content than out_room is
 * ZNIPPY_E_DST_SMALL.  Every member's CRC-32 is computed on the device from the bytes written and compared with its trailer, and its
 * ISIZE with the member's length mod 2^32: a mismatch on an otherwise clean item is ZNIPPY_E_CHECKSUM.  The first failure in stream
 * order decides the status; ZNIPPY_E_CHECKSUM is reported only if everything decoded.
 * Host validation and ZNIPPY_E_INVAL exactly as znippy_targz_find_batch (required: src_off, src_len, out_room, out_len; d_src, and d_out
 * when out_cap > 0); a room not inside out_cap is ZNIPPY_E_DST_SMALL; a src_len or room of 4 GiB or more is ZNIPPY_E_UNSUPPORTED.  The
 * call returns ZNIPPY_OK whatever the items report.
 * Writes: no byte of d_out outside the room of an item is written; inside the room of an item whose status is not 0 the bytes are
 * unspecified; rooms must not overlap (not checked).  A damaged file is a status, never a fault, a hang or a stray write.
 * Not a run, and synchronous on the context's stream, exactly as znippy_inflate_batch; no table is touched; every allocation (one,
 * sized from the source lengths: about 0.7 bytes per source byte and 3 KiB per item) is made before the first stream operation.
 * Stages (csrc/gunzip.hip, csrc/host/gz_plan.h; znippy_last_kernel_times: gunzip_scan, gunzip_probe, gunzip_single, gunzip_inflate,
 * gunzip_crc — only those that were launched):
 *   scan     finds candidate starts: every position behind 00 00 FF FF (a flush candidate) and every 1F 8B 08 (a member candidate,
 *            always kept).  A flush candidate closer than seg_min to the candidate kept before it (byte 0 is one) is dropped.
 *   probe    one wave per kept candidate decodes symbols and stored-block lengths and writes nothing.  It stops at the first block
 *            boundary that is a kept flush candidate, at its member's trailer, on an error or beyond the room, and records where it
 *            ended, the bytes it would produce and how far its matches reach in front of its first byte.
 *   plan     (host) walks each item's chain of records from byte 0.  Only candidates the chain lands on count, so the pattern inside
 *            compressed or stored data changes no result.  A piece whose matches reach back (a sync flush) joins the run in front of
 *            it; a run never crosses a member.
 *   inflate  one wave per run decodes into the final place, to the run's exact byte count.  Runs of no bytes are not launched.
 *   crc      the CRC launch of znippy_inflate_batch, a workgroup per run; the host combines the CRCs of a member's runs (as zlib's
 *            crc32_combine) and compares with the trailer.
 * An item without a kept candidate behind byte 0 (a crate, an sdist: one member, no flush) is decoded once, not twice: one wave
 * inflates it with the room as its limit and checks trailer and padding (single), its CRC goes to the crc launch, and a batch of such
 * items launches no probe.  The same wave takes, member by member, an item whose candidates outnumber its slice of the list
 * (16 + src_len / 256), so that no result depends on which candidates could be kept.
 * Opt-in (znippy_ctx_set_gunzip_cut below): block starts found inside streams without flush points, and the pieces between them
 * decoded in parallel from their predecessors' last 32 KiB.  bzip2 files: znippy_bunzip2_batch below; xz files: znippy_unxz_batch; listing the members of the tar inside: znippy_tar_list_batch. */
int znippy_gunzip_batch(znippy_ctx *ctx, const void *d_src, uint64_t src_cap, const uint64_t *src_off, const uint64_t *src_len, uint64_t n,
                        void *d_out, uint64_t out_cap, const uint64_t *out_off, const uint64_t *out_room, uint64_t seg_min, uint64_t *out_len,
                        int32_t *status, uint32_t *members, uint32_t *segments);

/* Cutting gzip files at block starts: opt-in, off by default.  A file whose writer left no cut points (a crate, an sdist, plain gzip
 * or zlib output, a log) can only be cut where a DEFLATE block starts, and block starts have to be found: at any bit offset, by
 * testing for a valid header; and a piece cut there reaches into bytes that do not exist yet.  With a value set, later
 * znippy_gunzip_batch calls of the context run these stages between scan and probe (znippy_last_kernel_times: gunzip_find,
 * gunzip_cut_probe, gunzip_decode, gunzip_tails, gunzip_apply, gunzip_cut_crc):
 *   find     every item of at least 2 * cut_bytes source bytes is tested at every bit position, a lane per position.  A position
 *            passes exactly when a non-final dynamic block (BFINAL 0, BTYPE 2) whose header satisfies the dynamic-block rules written
 *            at znippy_inflate_batch, up to its first body symbol, starts there inside the input (csrc/gz_cut_rules.h, one text for
 *            the kernel and for a host test).  The item's source is divided into windows of cut_bytes bytes counted from its byte 0;
 *            the lowest passing position of a window is its kept block candidate, so an item has ceil(src_len / cut_bytes) slots and
 *            the list cannot overflow.
 *   probe    one wave per candidate of an item the search kept a candidate in — byte 0, the kept block candidates, and the member and
 *            kept flush candidates of the scan —, as the probe above, with a piece starting at any bit and ending in front of the
 *            first block whose header starts at a kept candidate, flush or block; positions are 64-bit bit positions.
 *   plan     (host, csrc/host/gz_cut_plan.{h,cc}) the chain rule, member by member: only candidates the chain from byte 0 lands on
 *            count, so a false candidate changes no result.  A piece that reaches back does not join the piece in front: it becomes
 *            a marker piece — unless its symbols alone exceed the scratch budget: then it joins the run in front, as above.  A
 *            member's first piece and pieces that reach nowhere are decoded straight into place.  A reach beyond the member's first
 *            byte is "too far back".  Offsets are prefix sums of the probe's exact counts; consecutive pieces form passes whose
 *            marker pieces fit the scratch budget.  Nothing in a record is trusted.  The plan answers for files that are clean, and
 *            hands every other file — an error, a room too small, a wrong ISIZE, a reach too far back, garbage behind a trailer, any
 *            contradiction — to the stages behind, untouched, which decode it as with the value 0 and report what it is.
 *   decode   one wave per piece.  A marker piece goes to scratch as 16-bit symbols, 2 bytes per content byte: a value below 256 is
 *            a byte, 0x8000 | k names byte k of the 32,768 in front of the piece's first byte; matches inside the piece copy
 *            symbols, markers included, overlapping ones too.
 *   tails    one workgroup per item and pass takes the item's pieces in chain order and turns the last 32 KiB of each marker piece
 *            into bytes at their final place, reading markers from the final bytes in front of the piece.  The only serial loop runs
 *            inside one workgroup and is bounded by the piece count; no workgroup waits for another; a pass starts from the bytes
 *            earlier passes left.
 *   apply    every remaining symbol of every marker piece becomes a byte, a lane per symbol.
 *   crc      the CRC launch over the pieces, combined per item on the host and compared with the trailer; an item whose pieces or
 *            CRC are not clean is decoded again by the stages behind.
 * The contract is equivalence: out_len, status, members and, for status 0, the bytes in the room are those of the value 0, for every
 * input, damaged ones included.  segments keeps its meaning — the pieces of the item that a wave of its own decoded — and so grows
 * for a file that is cut; a file with flush points or members keeps every cut point it has with the value 0.  The lists of these
 * stages (about 180 bytes per slot and per entry of the scan's list) and the symbol scratch are three further allocations, made with
 * the first before the first stream operation.  A call whose searched items would need more than 2^30 slots, or whose further
 * allocations the device has no memory for, runs as with the value 0.
 *   cut_bytes   0 = off; 64 .. 2^30; anything else is ZNIPPY_E_INVAL.  ZNIPPY_GZ_CUT (0, or 64 ..) in the environment of
 *               znippy_ctx_create sets the initial value; a value that is not valid there is ignored.  znippy_ctx_gunzip_cut returns
 *               the value (0 for a NULL or closed context).  ZNIPPY_GZ_CUT_DEFAULT is the value the tools turn the switch on with: the largest of the
 *               best values swept at 8 and 64 MiB (4, 8 and 16 KiB are equal, 32 KiB and more slower; on one 512 MiB file, where
 *               the tails stage is four fifths of the call, 128 KiB is 1.8 times faster: profiles/gunzip_cut_report.log).
 *   ZNIPPY_GZ_CUT_SCRATCH_MB (read per call, default 1024, at least 1): the symbol scratch of one pass, never more than twice the
 *               rooms of the searched items.
 * znippy_ctx_gunzip_cut_stats describes the context's last znippy_gunzip_batch call (all zero after a call with the value 0):
 *   out[0]  bit positions tested: 8 * src_len of every searched item
 *   out[1]  positions that passed the whole header test
 *   out[2]  block candidates kept: windows with a passing position
 *   out[3]  kept candidates the chain landed on, block or flush, in the items that were cut
 *   out[4]  pieces decoded with markers        out[5]  pieces decoded straight into place
 *   out[6]  marker symbols resolved (3 to 6: of the items these stages finished)            out[7]  passes
 * Not done: cuts inside a block, stored-block or fixed-block candidates, the same for znippy_inflate_batch and ZIP entries. */
#define ZNIPPY_GZ_CUT_DEFAULT 16384ull
int znippy_ctx_set_gunzip_cut(znippy_ctx *ctx, uint64_t cut_bytes);
uint64_t znippy_ctx_gunzip_cut(const znippy_ctx *ctx);
int znippy_ctx_gunzip_cut_stats(znippy_ctx *ctx, uint64_t out[8]);

/* ---- whole bzip2 files the engine already holds --------------------------------------------------------------------------------
 * The bunzip2 of the reference's ingest side: host_decompress codec 2 and the tar.bz2 archive format of host_archive_open
 * (znippy-common/src/plugins/wasm_loader.rs:L18-31, L213-221, L410-441; design.md: "Bzip2 | lbzip2-rs | workers per core"): .bz2
 * files, .tar.bz2 / .tbz / .tbz2 source tarballs and older sdists, planet.osm.bz2 (TODO_NOW.md:L158, L400-407), all of which sit in the
 * archive as stored rows.  bzip2 blocks are independent: lbzip2 finds them by their 48-bit magic at any bit offset and decodes them
 * in parallel, and so does this call, a wave or a workgroup per block.
 *   d_src, src_cap     DEVICE: the region that holds the files; item i is the whole file d_src[src_off[i] .. + src_len[i])
 *   d_out, out_cap     DEVICE: item i's content goes to d_out[out_off[i] .. + out_room[i]), its room
 *   out_off            HOST, optional (NULL: the rooms lie back to back in array order)
 *   out_room           HOST: the bytes item i may produce.  bzip2 names the content's size nowhere: measure mode says it
 *   slot_cap           the most candidate blocks decoded per pass (below).  0 = the default: what fits a scratch budget of 1 GiB,
 *                      which ZNIPPY_BZ_SCRATCH_MB (a decimal number of MiB) replaces for every call.  A slot holds one block in front
 *                      of and behind the inverse BWT and its successor array: about 5 x level x 100,000 bytes are in use, and since the
 *                      level of a candidate ahead of the chain is not known when it is decoded every slot is sized for level 9
 *                      (6 x 900,000 bytes).  If not one slot fits the budget the call returns ZNIPPY_E_NOMEM with nothing queued.
 *                      No result depends on slot_cap.
 *   out_len            HOST out: bytes produced; 0 for every status but 0
 *   status             HOST, optional: per item, see below
 *   streams            HOST out, optional: bzip2 streams decoded (status 0)
 *   blocks             HOST out, optional: blocks decoded (status 0)
 * Measure mode: with d_out NULL and out_cap 0 nothing is written and out_room is not read; out_len[i] is the size the content has
 * (reported for status 0 only).  Statuses are as below, except that no CRC is checked and ZNIPPY_E_DST_SMALL cannot occur.
 * Per item, with Python's bz2.decompress as arbiter for everything it accepts: the content of all streams, concatenated; an item of
 * no bytes has no stream and no content (status 0).
 * Streams: the first must start with "BZh" and a digit 1-9, else ZNIPPY_E_CORRUPT.  Behind a stream's end (the end magic
 * 0x177245385090, the combined CRC, padding to a byte) a rest that starts with the three bytes "BZh" is another stream and is judged
 * like the first; any other rest, zeros included, is ignored, as the bzip2 tool and the arbiter do.  One stated deviation: the
 * arbiter silently drops a damaged later stream; this call reports it.
 * Blocks: a randomised block is ZNIPPY_E_UNSUPPORTED (no writer has set that bit since 0.9.5).  ZNIPPY_E_CORRUPT: input that ends
 * early; origPtr >= the block length; nGroups outside 2..6; nSelectors 0; a selector MTF index >= nGroups; a code length outside
 * 1..20 during the delta walk; an over-subscribed code, or a bit pattern no code has; a run (RUNA/RUNB) or a symbol count beyond
 * level x 100,000; a block of no symbols (or no used byte); the selectors running out; a block not followed by either magic.
 * nSelectors above 18002 is accepted, as bzip2 1.0.8 does: the surplus is read and discarded.  A block whose last bytes are four
 * equal ones without their count is accepted (the arbiter refuses it; no writer produces it).
 * Room and checksums: more content than out_room is ZNIPPY_E_DST_SMALL.  Every block's CRC (the bzip2 CRC-32: polynomial 0x04C11DB7,
 * MSB first), computed on the device from the bytes written, is compared with its header, and every stream's combined CRC
 * (c = rotl(c, 1) ^ block_crc) with its trailer: a mismatch on an otherwise clean item is ZNIPPY_E_CHECKSUM.  The first failure in
 * stream order decides the status.
 * Host validation and ZNIPPY_E_INVAL exactly as znippy_gunzip_batch (required: src_off, src_len, out_len, and out_room unless in
 * measure mode; d_src, and d_out when out_cap > 0); a room not inside out_cap is ZNIPPY_E_DST_SMALL; a src_len or room of 4 GiB or
 * more is ZNIPPY_E_UNSUPPORTED.  n == 0 is ZNIPPY_OK.  The call returns ZNIPPY_OK whatever the items report.
 * Writes: no byte of d_out outside the room of an item is written; inside the room of an item whose status is not 0 the bytes are
 * unspecified; rooms must not overlap (not checked).  A damaged file is a status, never a fault, a hang or a stray write.
 * Not a run, and synchronous on the context's stream, exactly as znippy_gunzip_batch; no table is touched; both allocations (the
 * lists: about 1.5 bytes per source byte; the slots) are made before the first stream operation, and ZNIPPY_POISON fills both.
 * Stages (csrc/bunzip2.hip, csrc/host/bz_plan.h; znippy_last_kernel_times: bunzip2_scan, bunzip2_decode, bunzip2_walk,
 * bunzip2_expand, bunzip2_crc — only those that were launched; decode to crc once per pass):
 *   scan     a wave covers 4 KiB of source: every bit position where the block magic 0x314159265359 starts goes to the candidate
 *            list.  The magic overlaps itself only at a shift of 45 bits, so an item holds at most 8 x src_len / 45 + 1 of them:
 *            the list is that long and has no overflow path.
 *   decode   one wave per job of the pass.  A stream header: "BZh", the level, the magic behind it.  A candidate block: CRC, origPtr,
 *            used-byte map, selectors, code lengths, then the symbols in groups of 50 (Huffman, RUNA/RUNB, MTF) into the slot; it
 *            records the length, the bit where the block ended, the magic there and, behind an end magic, the combined CRC and the
 *            byte behind the padding.  The chain of symbols is serial.
 *   walk     one workgroup per block that decoded: the successor array by a stable counting sort over 32 slices; the chain from
 *            origPtr followed sublist by sublist (splitter list ranking: every node whose index is a multiple of the spacing, 256,
 *            which ZNIPPY_BZ_SPLIT replaces, starts a sublist); a chain that closes early (periodic input) is walked once and
 *            repeated; then the lengths of the final run-length step, slice by slice.
 *   plan     (host) walks each item's chain of records from the first stream header: a candidate counts only if the block in front
 *            of it ended exactly at its bit, an end magic leads to the next stream header or to the end.  Candidates the chain has
 *            passed are dropped undecoded.  No record is trusted: each is checked against the item and the chain.  It assigns the
 *            output offsets, folds the combined CRC and chooses the next pass's up to slot_cap candidates in position order.
 *   expand   one workgroup per block landed on: four equal bytes, then a count of 0..251 — into its final place, never beyond the
 *            block's exact byte count.  The state does not cross blocks.
 *   crc      one workgroup per block landed on, over the bytes written.
 * Out of scope: parallel Huffman decoding inside a block, randomised blocks, any bzip2 encoder.  xz files: znippy_unxz_batch below.  The members of the tar inside a
 * .tar.bz2 are listed by znippy_tar_list_batch below, from the decompressed bytes. */
int znippy_bunzip2_batch(znippy_ctx *ctx, const void *d_src, uint64_t src_cap, const uint64_t *src_off, const uint64_t *src_len, uint64_t n,
                         void *d_out, uint64_t out_cap, const uint64_t *out_off, const uint64_t *out_room, uint64_t slot_cap, uint64_t *out_len,
                         int32_t *status, uint32_t *streams, uint32_t *blocks);

/* ---- whole xz files the engine already holds -----------------------------------------------------------------------------------
 * .xz, .tar.xz and .txz — kernel and toolchain tarballs, distro packages, many source releases — are in the reference's skip lists
 * (and in index.py's and znippy_host.cpp's), so they sit in the archive as stored rows, and the reference has no decoder for them: its
 * ecosystem list (TODO_NOW.md, "Holger ecosystem") only names an LZMA-family decoder, lzip, beside lgz and lbzip2.  The arbiter here
 * is liblzma 5.2, through Python's lzma.decompress.  An xz file names the compressed and the uncompressed size of every block in the
 * index at the end of each stream, so every block's source range and output offset are known before a byte is decoded: all blocks of
 * all items are decoded in one launch, a wave per block, straight into place.  Inside a block LZMA2 is an adaptive range coder and
 * strictly serial: the call pays off for batches of files and for multi-block files (xz -T, pixz); a lone single-block file is one
 * wave's work and far slower than a CPU thread (profiles/unxz_report.log).
 *   d_src, src_cap     DEVICE: the region that holds the files; item i is the whole file d_src[src_off[i] .. + src_len[i])
 *   d_out, out_cap     DEVICE: item i's content goes to d_out[out_off[i] .. + out_room[i]), its room
 *   out_off            HOST, optional (NULL: the rooms lie back to back in array order)
 *   out_room           HOST: the bytes item i may produce; measure mode says how many its indexes claim
 *   out_len            HOST out: bytes produced; 0 for every status but 0
 *   status             HOST, optional: per item, see below
 *   streams, blocks    HOST out, optional: streams and blocks decoded (status 0)
 *   unverified         HOST out, optional: the blocks of the item (status 0) whose integrity check was not verified, see Checks
 * Measure mode: with d_out NULL and out_cap 0 nothing is written and out_room is not read; out_len[i] is the sum of the uncompressed
 * sizes in the item's indexes.  No block header and no block data is read: the statuses come from the container walk alone, and
 * ZNIPPY_E_DST_SMALL cannot occur.  This is the file's claim, which a full call verifies block by block.
 * Container (xz file format 1.1.0).  An item is a sequence of streams, each optionally followed by stream padding (zero bytes, a
 * multiple of four); an item of no bytes has no stream and no content (status 0).  It is walked from its end, as xz --list does: the
 * footer (magic "YZ", CRC32 over backward size and flags), the index the backward size points at (indicator 0x00, record count,
 * unpadded / uncompressed size pairs as VLIs, zero padding, CRC32), the stream header at index start - sum of the padded block sizes
 * - 12, whose flags must equal the footer's, then the stream in front of that.  ZNIPPY_E_CORRUPT: any magic, CRC32 or padding that
 * is not as said, a VLI longer than 9 bytes or with a needless trailing zero byte, a record with an unpadded size below 5, a record
 * count the index bytes cannot hold, sizes that do not add up to the item, header and footer flags that differ, stream padding in
 * front of the first stream, bytes behind the last stream that are not stream padding.  ZNIPPY_E_UNSUPPORTED: a reserved flag bit,
 * content of 4 GiB or more.  ZNIPPY_E_DST_SMALL: more content than the room; nothing of that item is decoded.
 * Two deviations from lzma.decompress, both towards the xz tool: lzma.decompress drops whatever follows stream padding
 * (lzma.decompress(a + bytes(4) + b) is a's content alone), refuses padding behind the last stream, and ignores trailing bytes that
 * are no stream; the xz tool decodes both streams, accepts the padding and refuses the garbage, and so does this call.
 * Blocks.  The header: size byte, flags, optional compressed and uncompressed size, the filter list, zero padding, CRC32 (checked
 * first: a damaged header is ZNIPPY_E_CORRUPT whatever its fields say); sizes that are present must be the index's.  Exactly one
 * filter, LZMA2 (id 0x21, one property byte <= 40), is decoded; BCJ and delta filters, a filter chain, an unknown filter, a larger
 * property byte and a reserved header flag are ZNIPPY_E_UNSUPPORTED.  LZMA2 chunks: control 0x00 ends the block, 0x01 / 0x02 are
 * uncompressed chunks with / without a dictionary reset, 0x80-0xFF LZMA chunks (nothing / state reset / state reset + new properties
 * / + dictionary reset), 0x03-0x7F are corrupt.  The first chunk must reset the dictionary; the first LZMA chunk behind a dictionary
 * reset must bring properties; lc + lp <= 4 and a property byte <= 224.  An uncompressed chunk changes neither the LZMA state nor
 * what the next chunk must bring: behind 0x02 an LZMA chunk may go on with no reset at all (liblzma's rule, found with hand-built
 * chunk sequences).  The first byte of a chunk's range coder must be zero (liblzma checks it).  A chunk must consume exactly its
 * compressed and produce exactly its uncompressed size, the 0x00 must stand exactly at the end of the block's compressed size, the
 * output must be the index's uncompressed size, block padding must be zero.  An end marker inside LZMA2, a match that reaches in
 * front of the last dictionary reset and one beyond the declared dictionary size are corrupt: liblzma 5.2 draws both lines at the
 * same byte (its buffer is the declared size), so there is no deviation here.  All of these are ZNIPPY_E_CORRUPT.
 * Checks.  CRC32 (id 1) and CRC64 (id 4, ECMA-182 reflected, polynomial 0xC96C5795D7870F42) are computed on the device over the bytes
 * written and compared with the block's check field: a mismatch on an otherwise clean item is ZNIPPY_E_CHECKSUM.  With no check
 * (id 0), SHA-256 (id 10) and the reserved ids the content is delivered with status 0 and the block counts in `unverified`, as the xz
 * tool delivers it with a warning.  The first failure in stream order decides an item's status.
 * Host validation and ZNIPPY_E_INVAL exactly as znippy_bunzip2_batch (required: src_off, src_len, out_len, and out_room unless in
 * measure mode; d_src, and d_out when out_cap > 0); a room not inside out_cap is ZNIPPY_E_DST_SMALL; a src_len or room of 4 GiB or
 * more is ZNIPPY_E_UNSUPPORTED.  n == 0 is ZNIPPY_OK.  The call returns ZNIPPY_OK whatever the items report.
 * Writes: no byte of d_out outside the room of an item is written; inside the room of an item whose status is not 0 the bytes are
 * unspecified; rooms must not overlap (not checked).  A damaged file is a status, never a fault, a hang or a stray write.
 * Not a run, and synchronous on the context's stream, exactly as znippy_bunzip2_batch; no table is touched.  There is no scratch slot
 * per block, hence no slot_cap.  The tail stage's lists and staging buffer (72 bytes and at most 1,040 staged bytes per item) are
 * allocated before the first stream operation; a later round that asks for more, a long index, takes a larger staging buffer
 * (index bytes <= source bytes: a round never stages more than the source holds); the job lists (72 bytes per block), whose size
 * only the walk gives, are allocated when the rounds are over and the stream is idle.  ZNIPPY_POISON fills them all.
 * Stages (csrc/unxz.hip, csrc/host/xz_plan.h; znippy_last_kernel_times: unxz_tail once per round, unxz_decode, unxz_check — only
 * those that were launched):
 *   tail     a wave per byte range the host's container walk asks for; one copy back per round.  The first round brings every
 *            item's last 1 KiB and its first 12 bytes, which hold footer, index and header of most one-stream files: a batch of
 *            those takes one round; a stream in front of another, a longer index or long padding takes a round more each.
 *   plan     (host) all parsing, every container rule, the block job list (source range, output offset, declared sizes, check id)
 *            and the judgement of the decode records.  No byte and no record from the device is trusted: each is checked against
 *            the item and the index.
 *   decode   one wave per block: its own block header, the LZMA2 chunks, the range decoder in wave-uniform control flow (range,
 *            code, state and rep0-3 in scalars, probabilities as 16-bit cells in LDS, input through an LDS window), literals stored
 *            64 at a time, matches and uncompressed chunks copied by all lanes.  28,560 bytes of LDS per wave: five blocks per CU.
 *   check    one workgroup per block with check id 1 or 4, over the bytes written.
 * Out of scope: any xz or LZMA encoder, .lzma (LZMA-alone) and .lz (lzip) files, BCJ and delta filters, SHA-256 verification,
 * parallelism inside a block.  The members of the tar inside a .tar.xz are listed by znippy_tar_list_batch below, from the
 * decompressed bytes. */
int znippy_unxz_batch(znippy_ctx *ctx, const void *d_src, uint64_t src_cap, const uint64_t *src_off, const uint64_t *src_len, uint64_t n,
                      void *d_out, uint64_t out_cap, const uint64_t *out_off, const uint64_t *out_room, uint64_t *out_len, int32_t *status,
                      uint32_t *streams, uint32_t *blocks, uint32_t *unverified);

/* ---- the members of tars held in device memory ------------------------------------------ */
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
/* Every regular member of n tars — what the reference's tar_entries_from_bytes (wasm_loader.rs, host_archive_open formats 1 and 2)
 * returns for a decompressed .tar.gz / .tar.bz2 — listed and, where wanted, extracted on the device.
 * Item i is the tar d_tar[tar_off[i] .. + tar_len[i]) (DEVICE, any alignment; below 4 GiB each): a plain tar, or what
 * znippy_gunzip_batch / znippy_bunzip2_batch made of a compressed one.  Listed are the members of typeflag '0', '\0' (unless the name
 * field ends with '/': a V7 directory) and '7', in stream order, whose name starts with name_prefix and ends with name_suffix (bytes,
 * compared as such; empty = all; the filter of znippy_targz_find_batch).  The name is the pending GNU 'L' name or pax path= (of several
 * in front of one member the first), else prefix "/" name, else name.  'g' and 'K' entries are stepped over; one zero block is stepped
 * over, two end the tar, and so does the end of the item's bytes at a header boundary with no name pending (csrc/tar_list_rules.h).
 *   members      HOST, members_cap entries.  The matching members of item i are members[member_first[i] .. member_first[i + 1]);
 *                header_off, data_off and size are relative to the item's first byte.
 *   names        HOST, names_cap bytes: the names, packed in member order, not terminated
 *   d_out        DEVICE, out_cap bytes, or NULL with out_cap 0: the members' bytes, packed in member order at out_off (without d_out,
 *                out_off says where they would stand)
 *   member_first HOST, n + 1.   names_bytes, out_bytes: HOST, the bytes of names and of d_out the listed members take
 *   status       HOST, optional: 0 or ZNIPPY_E_* per item
 * Measure mode: members NULL with members_cap 0 (names and d_out NULL as well).  Nothing is written but member_first, *names_bytes
 * and *out_bytes, which are what a full call with caps that hold everything reports.
 * Per item: ZNIPPY_E_CORRUPT — a block on the chain from byte 0 that is neither zero nor a valid header (checksum, unsigned or
 * signed), a size field that is no number, a header, payload or member (with its padding) that crosses the item's end, a pending
 * name with no member behind it, a malformed pax record.  ZNIPPY_E_UNSUPPORTED — a GNU sparse member, an 'L' / 'x' payload above
 * 8 KiB, an item of 4 GiB or more, and the two deviations from `tarfile`: (1) a pax size= record that differs from the size field
 * of the member behind it (one that equals it is accepted; writers emit a differing one only for members of 8 GiB and more);
 * (2) more than 64 extended headers ('L', 'x', 'X', 'g', 'K') in a row with no member or zero block between them (writers emit
 * four at most; the bound keeps the emit stage's look back short whatever the input is).  A wrong offset is never listed.  ZNIPPY_E_DST_SMALL — the item's members, names or contents no longer fit a cap: the item takes no room,
 * and items behind it may still fit.  ZNIPPY_E_INVAL — the item does not lie inside tar_cap.  An item with a status lists no member
 * (the reference's `.ok()?`).  A tar nested in a member, headers behind the two zero blocks and member data that looks like a header
 * are judged and never reached: they add nothing.
 * The call returns ZNIPPY_OK whatever the items report; n == 0 is ZNIPPY_OK.  ZNIPPY_E_INVAL: NULL member_first, names_bytes,
 * out_bytes, tar_off, tar_len or d_tar, a cap without its buffer, a filter string of 64 KiB or more, measure mode with names or d_out.
 * Writes: no entry of members, byte of names or byte of d_out outside what member_first, *names_bytes and *out_bytes report.
 * Not a run, and synchronous on the context's stream, exactly as znippy_gunzip_batch; no table is touched; the allocations (the
 * per-block lists: about 37 bytes per 512-byte block; staging for records, names and gather pieces, bounded by the caps) are made
 * before the first stream operation, and ZNIPPY_POISON fills them.
 * Stages (csrc/tar_list.hip, csrc/host/tar_list_plan.h; znippy_last_kernel_times: tar_scan, tar_chain, tar_emit, tar_emit_write,
 * tar_gather — only those that were launched):
 *   scan     a half-wave per 512-byte block, 16 bytes a lane: zero test and checksum by a reduction, and for a block whose checksum
 *            holds the header's kind, size and successor (an 'L' / 'x' / 'X' header with its payload).  A dense record per block:
 *            no overflow path.  Terminals — the first of two zero blocks, no header, unsupported, a step past the end — lead to
 *            themselves.
 *   chain    rounds of pointer doubling over all blocks of all items: a marked block marks the target of its jump pointer, and the
 *            jump pointers square.  The number of rounds is ceil(log2(blocks of the largest item + 1)), whatever the tars hold.
 *   emit     every marked member header looks back over the extended headers directly in front of it for its name and for a
 *            differing size=; the first failing block in stream order is the item's status; members that pass the filter are counted
 *            (prefix sums over chunks of 256 blocks).  The host turns the totals into statuses and room (caps), and a second launch
 *            writes records and names to staging lists.  The host checks every record against its item before it reaches the caller
 *            or becomes a piece of the gather: no device record is trusted.
 *   gather   the contents, by the range reads' gather, only with d_out. */
int znippy_tar_list_batch(znippy_ctx *ctx, const void *d_tar, uint64_t tar_cap, const uint64_t *tar_off, const uint64_t *tar_len, uint64_t n,
                          const char *name_prefix, uint64_t prefix_len, const char *name_suffix, uint64_t suffix_len,
                          znippy_tar_member *members, uint64_t members_cap, char *names, uint64_t names_cap,
                          void *d_out, uint64_t out_cap, uint64_t *member_first /* n + 1 */, uint64_t *names_bytes, uint64_t *out_bytes,
                          int32_t *status);

/* ---- (2)+(4) batch encode + hash over Rounds -------------------------------------------- */
/* A Round is (offset,len,skip) into one staging buffer (slotpool.rs:L39-47,
 * stream_packer.rs:L98-106).  HOST arrays, n entries.  src_offset is a full 64-bit value and rounds may share or overlap
 * source bytes; for sizes see "What may exceed 4 GiB" at znippy_rows_create. */
int znippy_rounds_create(znippy_ctx *ctx, const uint64_t *src_offset, const uint64_t *len,
                         const uint8_t *skip, uint64_t n, znippy_rounds **out);
void znippy_rounds_destroy(znippy_rounds *rounds);
/* Opt-in content-based store path (the reference's wish list, TODO_NOW.md:L37-38):
 * a round whose frame would not be smaller than its input is emitted as-is with compressed = 0.
 * OFF by default — the reference decides by file extension only (index.rs:L470-488), so turning this
 * on changes the `compressed` column for incompressible rounds. */
int znippy_rounds_set_store_incompressible(znippy_rounds *rounds, int on);
/* Opt-in aligned blob offsets (what zipalign does for zip): every payload of later znippy_encode_hash_rounds[_async]
 * calls on this table starts at a multiple of `align` — a power of two in 1 .. 4096; 1, the default, packs back to back.
 * Anything else, a NULL table or a closed context gives ZNIPPY_E_INVAL and changes nothing.  Runs already queued keep
 * the value they were queued with, also while two runs are in flight.  With align = a:
 *   blob_offset[0] = 0, blob_offset[i+1] = round_up(blob_offset[i] + blob_size[i], a);
 *   blob_size[i] is the payload alone, and the payload's bytes are those of the packed run (frames do not depend on a);
 *   *blob_bytes = blob_offset[n-1] + blob_size[n-1]: no padding behind the last round;
 *   the gap bytes between payloads are written as zero; no byte at or beyond *blob_bytes is written;
 *   an empty payload sits at an aligned offset of its own, and the next round starts there too.
 * znippy_rounds_blob_bound follows the setter (the packed bound + (n - 1) * (a - 1)); a region smaller than the run
 * needs gives ZNIPPY_E_DST_SMALL as on the packed path, with nothing written outside [0, blob_cap).  Offsets are relative
 * to d_blob_out: for absolute alignment, give an aligned base.  With a >= 16 and a 16-byte aligned d_blob_out a
 * store-heavy table's hash + copy pass always runs its aligned form (which gains where the destinations are whole 128-byte
 * lines: 128 is the value for that; 4096 is for direct I/O and mapping).  The row table of such an archive is not "front to
 * back": readers get its offsets from the blob_offset column, as for any index. */
int znippy_rounds_set_blob_align(znippy_rounds *rounds, uint32_t align);
uint32_t znippy_rounds_blob_align(const znippy_rounds *rounds); /* 1 for a NULL table */
/* Opt-in block tree from the write side ("block tree" above): the hash of a round above 64 KiB already computes the non-root
 * chaining value of every 64 KiB tile, a 128 KiB block is two tiles, so one small kernel behind the hash (kernel time:
 * block_tree_entries) turns them into the entries of the archive rows these rounds become — no input byte is read a second time,
 * where znippy_rows_block_tree_build decodes and hashes every multi-block row whole.
 * znippy_rounds_emit_block_tree: OFF by default; applies to later znippy_encode_hash_rounds[_async] calls on this table; runs
 * already queued keep the setting they were queued with, also while two runs are in flight.  The first switch-on makes every
 * allocation the feature needs (no queueing call allocates for it): the list of rounds with entries and, per slot of the two-run
 * ring, a device tree buffer and a pinned host mirror.  With emission off no launch, allocation or result differs from a table that
 * was never asked.  A NULL table or a closed context gives ZNIPPY_E_INVAL.
 * znippy_rounds_block_tree_layout: znippy_rows_block_tree_layout with len = the round's source length; round_first (HOST, n + 1
 * values) is optional; works whether emission is on or off.
 * znippy_rounds_block_tree: the tree of the run `lag` (0 or 1) runs before the latest queued one, into `tree` (HOST, 32 * n_entries
 * bytes; may be NULL when n_entries is 0).  The tree leaves on the copy stream with that run's results and the call waits for that
 * copy only.  ZNIPPY_E_INVAL if there is no such run or it was queued with emission off.
 * The entries are byte for byte what znippy_rows_block_tree_build returns for those rows: they depend on the source bytes alone —
 * not on level, window, store_incompressible, blob alignment or the hash route.  znippy_hash_rounds emits nothing. */
int znippy_rounds_emit_block_tree(znippy_rounds *rounds, int on);
int znippy_rounds_block_tree_layout(znippy_ctx *ctx, znippy_rounds *rounds, uint64_t *n_entries, uint64_t *round_first);
int znippy_rounds_block_tree(znippy_ctx *ctx, znippy_rounds *rounds, unsigned lag, uint8_t *tree);
/* Upper bound of the blob bytes znippy_encode_hash_rounds can produce for this batch. */
uint64_t znippy_rounds_blob_bound(const znippy_rounds *rounds);

/* For every round: checksum = BLAKE3(src slice) (pre-compression bytes); skip -> the raw bytes
 * are the payload (compressed=0), else one zstd frame (compressed=1).  Payloads are packed
 * back-to-back from d_blob_out[0] in round order (blob offsets are a running sum — the
 * writer's out_cursor.fetch_add, stream_packer.rs:L258).
 *   d_src      : DEVICE staging buffer the rounds point into
 *   d_blob_out : DEVICE, blob_cap bytes (>= znippy_rounds_blob_bound)
 *   HOST outputs, n entries each: blob_offset, blob_size (= on_disk_len), checksum (32 B each),
 *   compressed (0/1).  *blob_bytes = total payload bytes. */
int znippy_encode_hash_rounds(znippy_ctx *ctx, znippy_rounds *rounds, const void *d_src,
                              void *d_blob_out, uint64_t blob_cap, uint64_t *blob_offset,
                              uint64_t *blob_size, uint8_t *checksum, uint8_t *compressed,
                              uint64_t *blob_bytes);
int znippy_encode_hash_rounds_async(znippy_ctx *ctx, znippy_rounds *rounds, const void *d_src,
                                    void *d_blob_out, uint64_t blob_cap);
int znippy_rounds_results(znippy_ctx *ctx, znippy_rounds *rounds, uint64_t *blob_offset,
                          uint64_t *blob_size, uint8_t *checksum, uint8_t *compressed,
                          uint64_t *blob_bytes);

/* Zero-copy results: pointers into the table's pinned host mirror (one D2H), valid until the next
 * encode call on the same table. */
int znippy_rounds_results_view(znippy_ctx *ctx, znippy_rounds *rounds, const uint64_t **blob_offset,
                               const uint64_t **blob_size, const uint8_t **checksum, uint64_t *blob_bytes);

/* The same for the run `lag` (0 or 1) runs before the latest one; waits for that run's result copy only (every
 * run's results leave on a copy stream into their own pinned mirror).  Pointers stay valid until two more encode
 * calls have been queued on the table. */
int znippy_rounds_results_lagged(znippy_ctx *ctx, znippy_rounds *rounds, unsigned lag, const uint64_t **blob_offset,
                                 const uint64_t **blob_size, const uint8_t **checksum, uint64_t *blob_bytes);

/* Hash only (store path / verify-only): digests[i] = BLAKE3(d_src[off_i .. off_i+len_i]).
 * digests: HOST, 32 bytes per round. */
int znippy_hash_rounds(znippy_ctx *ctx, znippy_rounds *rounds, const void *d_src, uint8_t *digests);

/* ---- measurement hooks (bench.py): device time of the last async call's kernels, by HIP
 * events on the stream each kernel was queued on.  names/ms: up to cap entries; returns the count.
 * A run queued on a run lane beside another run (see znippy_decode_verify_rows) has its events on that lane: the bracketed
 * kernel's time then includes its wait for CUs the earlier run still holds.  With nothing else in flight (queue, read the
 * results, ask) the times are the kernels' own. */
int znippy_last_kernel_times(znippy_ctx *ctx, const char **names, float *ms, int cap);
/* Run lanes, host-side counters since the context was created, by what the streams really order: out[0] lean runs queued
 * on the other stream than their predecessor with no wait for it (the only runs that can execute beside another), out[1]
 * lane runs behind their predecessor — by a wait for its event, by standing on the same stream, or with no lane run in
 * front of them —, out[2] lane runs in front of which a mark was recorded on the context's stream because other work had
 * been queued there, out[3] lean runs kept off the lanes (a caller's stream, ZNIPPY_NO_RUN_LANES, ZNIPPY_NO_FORK_VERIFY).
 * znippy_ctx_run_lane_older_waits (introspection for the tests only, not part of the stable interface): lane runs that were made to wait for a run OLDER than their predecessor which had not
 * ended on the other stream (a run only ever starts with nothing but its predecessor still executing).
 * Both queue nothing and wait for nothing. */
int znippy_ctx_run_lane_stats(znippy_ctx *ctx, uint64_t out[4]);
int znippy_ctx_run_lane_older_waits(znippy_ctx *ctx, uint64_t *out);
/* How many of those event pairs a call records: 2 = around every kernel (default), 1 = around the dominant read
 * kernels only (decode_verify_*), 0 = none (a caller that never asks for kernel times: each pair costs the stream
 * two markers).  ZNIPPY_KTIME in the environment sets the initial level. */
int znippy_ctx_set_kernel_timing(znippy_ctx *ctx, int level);
/* Statistics of the last run's two-phase path for foreign multi-block frames (frames another zstd writer produced;
 * codec.rs:L67-78 decodes whatever the archive holds): stats[0] literal-pool bytes and stats[1] sequence-pool records
 * handed out, stats[2] frames decoded by that path, stats[3] blocks it left to the serial decoder, of which stats[4]
 * for an error the serial decoder will report, stats[5] a Treeless / Repeat_Mode table more than 64 blocks back,
 * stats[6] a pool that ran out, stats[7] a value outside the record format.  Synchronises. */
int znippy_rows_foreign_stats(znippy_ctx *ctx, znippy_rows *rows, uint64_t stats[8]);
/* Content checksums on the batch path (opt-in, off by default).  A zstd frame may end with a Content_Checksum: 4 bytes, the
 * low 32 bits of XXH64 (seed 0) over its content (RFC 8878 3.1.1; `zstd` on the command line writes one by default).  With the
 * switch off such a frame is decoded and checked by the serial decoder, one workgroup per frame.  With it on, the read runs of
 * this context (decode + verify, decode-only, verify-only) take these frames through the batch and resolve paths like any other
 * foreign frame, and a stage behind them (kernel time name zstd_batch_checksum) hashes every frame that was decoded there and
 * compares it with the trailer.  A frame whose trailer differs is not reported by that stage: it is handed to the serial
 * decoder, which decodes it again and reports ZNIPPY_E_CHECKSUM for the row, as it does with the switch off — statuses, bytes
 * and counters of a run are the same either way.  Frames without a trailer, and every frame the batch path declines, go the way
 * they went.  The value is read at the start of every run: a table may be run with the switch on and off in turn.
 * on: 0 or 1; anything else, and a closed context, give ZNIPPY_E_INVAL.  ZNIPPY_BX_CHECKSUM=1 in the environment of
 * znippy_ctx_create sets the initial value.  znippy_ctx_batch_checksums returns the value. */
int znippy_ctx_set_batch_checksums(znippy_ctx *ctx, int on);
int znippy_ctx_batch_checksums(const znippy_ctx *ctx);
/* The checksum stage's counters of the table's last run: stats[0] frames whose trailer it checked and found right, stats[1]
 * frames it checked and found wrong (handed to the serial decoder), stats[2] content bytes it hashed, stats[3] 0.  All zero
 * for a run with the switch off.  Synchronises. */
int znippy_rows_checksum_stats(znippy_ctx *ctx, znippy_rows *rows, uint64_t stats[4]);
/* The hash's VALU floor, measured: nanoseconds one 64-lane BLAKE3 compress pass costs a SIMD when nothing else runs
 * (a kernel of compressions only, 4 waves per SIMD on every CU), and the shader clock that kernel held (may be NULL).
 * bench.py prices the read step's passes with it. */
int znippy_measure_blake3_pass_ns(znippy_ctx *ctx, float *ns_per_pass_per_simd, float *shader_ghz);
/* Shader clock (GHz) one wave of the read side's small-row kernel saw during the last run of a context created with
 * ZNIPPY_DBG bit 32768 set: its life in shader cycles / in 100 MHz ticks.  0 if nothing was recorded. */
int znippy_last_shader_ghz(znippy_ctx *ctx, float *ghz);
/* Diagnostic: the role-split read kernel as this library was built and as this context runs it.  geometry[0] waves per
 * workgroup, [1] ring slots, [2] workgroups per CU, [3] bytes of dynamic LDS per workgroup, [4] registers per lane, [5] LDS
 * bytes it holds of a CU, [6] 1 if a run's verify is queued beside the next run (it fits on a CU beside the kernel), [7] 1 if
 * the run lanes are on.  From a context created with ZNIPPY_DBG bit 32768 also what the waves of the last run left: 8 words
 * per wave, workgroup by workgroup (word 7 of each: the launch's workgroups) — its life in shader cycles; the cycles of its
 * three waits (a hasher: before its first tile, between tiles, the last one that ends without a tile; the loader: for a free
 * group, for its publish turn, and the length of its first iteration); the tiles (iterations) it got; its first and last
 * 100 MHz tick.  At most cap_words words are copied to waves (HOST; may be NULL with cap_words 0), *n_words says how many.
 * Synchronises. */
int znippy_roles_wait_stats(znippy_ctx *ctx, uint32_t geometry[8], uint64_t *waves, uint64_t cap_words, uint64_t *n_words);

/* Where a verify-only run (znippy_verify_rows) keeps the rows it has to materialise: the context's scratch region as it
 * is now (*d_base, DEVICE; NULL when the table needs none), the extent of this table's slots in it (*bytes) and, when
 * row_offset is not NULL, every row's slot (HOST, one entry per row of the table, UINT64_MAX = the row has no slot: a
 * stored or an empty row).  Builds the slots and the region if no verify run has yet.  For tests and measurements — the
 * region's contents are no contract for consumers, and the pointer moves when the region grows. */
int znippy_rows_verify_scratch(znippy_ctx *ctx, znippy_rows *rows, const void **d_base, uint64_t *bytes,
                               uint64_t *row_offset);

#ifdef __cplusplus
}
#endif
#endif /* ZNIPPY_HIP_H */
