/*
 * ntcomp_codec.h -- block container of encoded.dat (libntcomp_gpu.so).
 *
 *   ntc_file_header   encode_file_header(0,0,0,0)           src/lib.rs:52-67 (32 zero bytes)
 *   ntc_write_block   write_block_to(u64_encoding, num_records, sink)   src/lib.rs:232-252
 *                     (split_encoded_dictionary + compress_block x4, src/encode.rs:96-229)
 *                     = ntc_pack_block + ntc_deflate_block
 *   ntc_pack_block    the part of write_block_to before deflate: split_encoded_dictionary
 *                     (src/encode.rs:168-229), rice_encode / minimal_binary_encode
 *                     (src/encode.rs:59-94) and the bytes compress_block hands to
 *                     deflate_bytes (src/encode.rs:107-109), per stream
 *   ntc_pack_blocks_device
 *                     the same on the GPU, for every block of a batch of encoded reads
 *                     (records already in HBM, straight from ntc_encode_batch_device)
 *   ntc_deflate_block the rest of compress_block: gzip each stream (deflate_bytes,
 *                     src/encode.rs:49-57) and prefix its 32-byte BlockHeader
 *                     (src/lib.rs:37-50, src/encode.rs:113-120)
 *   ntc_read_block    decode_block's container half: 4 x (32-byte header, gzip payload),
 *                     decompress_block x4 + zip_block_contents      src/lib.rs:320-363,
 *                     src/decode.rs:79-149 -- returns the u64 records that
 *                     decode_sequence (ntc_decode_batch) consumes.
 * Buffers returned through uint8_t** / uint64_t** are freed with ntc_buffer_free.
 */
#ifndef NTCOMP_CODEC_H
#define NTCOMP_CODEC_H

#include <stdint.h>

#include "ntcomp_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One coded stream of a block, before deflate: 8 * encoded_size payload bytes at
 * `offset`, the u64 code words in the byte order compress_block gives deflate (each word
 * big-endian: the MSB-first bit stream of dsi-bitstream's BE BufBitWriter). */
typedef struct ntc_stream_meta {
    uint64_t num_u64;      /* values in the stream          (BlockHeader.num_u64)      */
    uint64_t encoded_size; /* u64 code words                (BlockHeader.encoded_size) */
    uint64_t param;        /* Rice log2_b, or minimal-binary max = max value + 2
                              (BlockHeader.rice_param)                                 */
    uint64_t offset;       /* byte offset of the payload in the caller's payload buffer */
} ntc_stream_meta;

/* The four streams of one block: [0] colex ranks (minimal binary), [1] match lengths
 * (Rice), [2] flag bytes (Rice), [3] short-record bases in 31-base 2-bit chunks (minimal
 * binary).  status = NTC_ERR_EMPTY_READ when s1 or s4 is empty: the reference's
 * minimal_binary_encode errs and write_block_to writes nothing (src/encode.rs:80,
 * src/lib.rs:242-250; main.rs:170 ignores the error -- SURVEY App. B.3).             */
typedef struct ntc_block_meta {
    ntc_stream_meta stream[4];
    uint64_t num_records; /* BlockHeader.num_records (reads in the block; main.rs:170,176) */
    uint64_t n_recs;      /* u64 records of the block                                   */
    int32_t status;
    uint32_t reserved;
} ntc_block_meta;

#define NTC_DEFLATE_ZLIB 0       /* system zlib, level 6                                  */
#define NTC_DEFLATE_LIBDEFLATE 1 /* libdeflate.so.0, level 6 (~3x faster; other deflate
                                    bytes, same inflated content)                       */
#define NTC_DEFLATE_ADAPTIVE 2   /* libdeflate level 6 where it compresses: a stream whose
                                    first 32 KiB carry >= 7.9 bits of order-0 entropy per
                                    byte (s1's colex ids and s4's bases are such: level 6
                                    shrinks them by < 0.1 %) goes out as stored deflate
                                    blocks, as zlib's own stored-block fallback would write
                                    it; half the CPU of NTC_DEFLATE_LIBDEFLATE, same streams
                                    after inflate, within 0.1 % of its size              */
#define NTC_DEFLATE_GPU 3        /* the coder of the device (deflate.hip):
                                    32 KiB chunks coded on their own, each stored, Huffman
                                    over literals, or Huffman over literals and greedy
                                    in-chunk matches, whichever is exactly smallest.  Here
                                    (ntc_deflate_block / _stream) its host restatement runs:
                                    the device's bytes, no libdeflate, no GPU.  Block streams
                                    only: the side-section deflaters refuse it.           */

void ntc_file_header(uint8_t out[32]);
/* NTC_ERR_EMPTY_READ when the block has no long or no short records (see above). */
int ntc_write_block(const uint64_t *recs, uint64_t n_recs, uint64_t num_records, uint8_t **out,
                    uint64_t *out_len);
/* Host packer: *payload (freed with ntc_buffer_free) holds the four streams back to back,
 * meta->stream[s].offset relative to it.  Returns meta->status.                       */
int ntc_pack_block(const uint64_t *recs, uint64_t n_recs, uint64_t num_records, ntc_block_meta *meta,
                   uint8_t **payload, uint64_t *payload_len);
/* Header + gzip member per stream, the bytes write_block_to writes.  payload is the base
 * the meta offsets are relative to.  engine: NTC_DEFLATE_ZLIB, _LIBDEFLATE, _ADAPTIVE
 * (NTC_ERR_UNSUPPORTED if libdeflate.so.0 is missing) or _GPU; any other value is
 * NTC_ERR_INVALID_ARG.  Returns meta->status when the
 * block is dropped (nothing written).                                                  */
int ntc_deflate_block(const ntc_block_meta *meta, const uint8_t *payload, int engine, uint8_t **out,
                      uint64_t *out_len);
/* One stream's part of ntc_deflate_block (its 32-byte header + gzip member): a block's
 * bytes are streams 0..3 concatenated, so a pool can deflate them in parallel.          */
int ntc_deflate_stream(const ntc_block_meta *meta, int stream, const uint8_t *payload, int engine, uint8_t **out,
                       uint64_t *out_len);
/* Parses one block at data[0..len).  NTC_ERR_IO on a clean end of input (no bytes left),
 * NTC_ERR_FORMAT on a damaged block (decode_block's Err, which ends the reference's
 * decode loop, src/main.rs:202).                                                      */
int ntc_read_block(const uint8_t *data, uint64_t len, uint64_t *consumed, uint64_t **recs,
                   uint64_t *n_recs, uint64_t *num_records);
/* The same into a caller buffer of capacity records (NTC_ERR_CAPACITY, with *n_recs the
 * block's count, when it does not fit).  Inflate through libdeflate when present.       */
int ntc_read_block_into(const uint8_t *data, uint64_t len, uint64_t *consumed, uint64_t *recs, uint64_t capacity,
                        uint64_t *n_recs, uint64_t *num_records);
void ntc_buffer_free(void *p);

/* ---- GPU packer ---------------------------------------------------------------------- */
/* Blocks of a batch of encoded reads: block b = reads [b * block_reads,
 * min((b + 1) * block_reads, n_reads)), num_records = its read count (the caller passes
 * block_reads = 65536, main.rs:152; a final partial block carries n_reads % 65536 as
 * main.rs:176 does).  d_recs / d_rec_offsets[n_reads + 1] are device buffers as
 * ntc_encode_batch_device writes them (offsets relative to d_recs).  Writes every
 * block's four payloads into d_payload (device, payload_capacity bytes) and n_blocks
 * metas into the HOST array meta (offsets relative to d_payload; each stream gets room
 * for an exact upper bound of its code, so payloads have small gaps).  *payload_bytes =
 * bytes used (on NTC_ERR_CAPACITY: bytes needed; about 1-2 B per record is typical).
 * Synchronous: the Rice parameters are computed on the host (glibc log/exp as the
 * reference's f64 math) from a first device pass.                                     */
int ntc_pack_blocks_device(ntc_ctx *ctx, const uint64_t *d_recs, const uint64_t *d_rec_offsets,
                           uint64_t n_reads, uint32_t block_reads, uint8_t *d_payload,
                           uint64_t payload_capacity, ntc_block_meta *meta, uint64_t *payload_bytes);
/* Host reads -> packed blocks in one call: ntc_encode_batch's device pass (one pass,
 * however many bases) + ntc_pack_blocks_device, so the u64 records never leave HBM: the
 * CLI's path (src/main.rs:162-177: encode_sequence + encode_dictionary per read, then
 * write_block_to per 65,536 reads, up to deflate).  meta: ceil(n_reads / block_reads)
 * entries.  *payload (host, freed with ntc_buffer_free) holds every block's streams at
 * the meta offsets; hand each block to ntc_deflate_block.                              */
int ntc_encode_pack_batch(ntc_ctx *ctx, const uint8_t *bases, const uint64_t *read_offsets, uint64_t n_reads,
                          uint32_t block_reads, ntc_block_meta *meta, uint8_t **payload, uint64_t *payload_bytes,
                          int64_t *bad_read);

/* ---- GPU deflate (NTC_DEFLATE_GPU on the device) ---------------------------------------- */
/* The gzip members of n_blocks packed blocks, made where the packer left them: d_payload
 * (device) and the HOST metas as ntc_pack_blocks_device gives them.  Stream s of block b
 * becomes one member in d_out (device, out_capacity bytes), the members back to back;
 * member_off_len (host, 4 pairs per block) says where each starts in d_out and how many bytes
 * it has.  The bytes are those of ntc_deflate_stream with NTC_DEFLATE_GPU, less its 32-byte
 * stream header.  A block whose status is not 0 yields nothing (pairs of zeros); an empty
 * stream yields a member that inflates to nothing.  *out_bytes = bytes used.  A capacity below
 * the sum over the streams of 18 + n + 5 ceil(n / 32768) + 5 (n = 8 encoded_size) is
 * NTC_ERR_CAPACITY with *out_bytes = that sum; nothing was launched.  Synchronous.           */
int ntc_deflate_blocks_device(ntc_ctx *ctx, const uint8_t *d_payload, const ntc_block_meta *metas, uint64_t n_blocks,
                              uint8_t *d_out, uint64_t out_capacity, uint64_t *member_off_len, uint64_t *out_bytes);
/* ntc_ctx_set_option(ctx, "gpu_deflate", 1) (default 0: nothing is launched, no byte or copy
 * changes) makes ntc_encode_pack_batch, ntc_encode_pack_fastq and ntc_encode_pack_fastq_paired
 * run that pass behind the packer: *payload then holds the members, not the raw streams, which
 * never leave the device, and the meta offsets no longer apply.  ntc_encode_members fetches
 * where they lie, 4 pairs (offset in *payload, bytes) per block, zeros for a dropped block:
 * what the last such call on this context left, to be fetched before the next one, like
 * ntc_encode_digests.  *n_blocks = the call's blocks (0 when the option was off);
 * NTC_ERR_CAPACITY when cap_blocks is smaller.                                             */
int ntc_encode_members(ntc_ctx *ctx, uint64_t *member_off_len, uint64_t cap_blocks, uint64_t *n_blocks);

/* ---- GPU inflate of gzip members of at most 64 KiB (BGZF) -------------------------------- */
/* Member i is the src_bytes bytes at comp + src_off: one whole gzip member (RFC 1952 with any
 * of FEXTRA, FNAME, FCOMMENT, FHCRC; RFC 1951 with any number of stored, fixed and dynamic
 * blocks) that fills those bytes exactly and inflates to exactly out_bytes <= 65,536 bytes,
 * which go to dst + dst_off.  Each member is decoded on its own (inflate.hip: one workgroup per
 * member) and its CRC-32 and ISIZE are checked there.  res[i].status:
 *   0 sound: out_bytes bytes written, crc their CRC-32
 *   1 bad header (magic, method, a reserved flag bit, the header's CRC16)
 *   2 bad block (type 3, stored LEN != ~NLEN, HLIT > 286, HDIST > 30)
 *   3 bad code (what zlib's inflate_table refuses, no end-of-block code, a bad repeat, bits that
 *     are no code, length symbols 286/287, distance symbols 30/31)
 *   4 bad distance (past the bytes produced so far)
 *   5 output overrun (the member holds more than out_bytes)
 *   6 input overrun (bits needed past src_bytes, or bytes left behind the trailer)
 *   7 CRC mismatch      8 ISIZE mismatch (against out_bytes or the bytes produced)
 *   9 too large (out_bytes > 65,536; nothing was looked at)
 * A member whose status is not 0 writes nothing to dst: no failure touches another member's
 * bytes or its own.  *n_failed = the members with a status other than 0.  The call returns
 * NTC_OK when it ran, whatever the statuses.  NTC_ERR_INVALID_ARG, before anything is launched:
 * a null argument, a member outside comp[0, comp_bytes) or dst[0, dst_cap), two members whose
 * dst ranges overlap, n >= 2^31.
 *   ntc_inflate_members         host to host through the GPU; with ctx == NULL the decoder's
 *                               host restatement runs (the same function with one lane): the
 *                               device's bytes and statuses, no GPU
 *   ntc_inflate_members_device  d_comp and d_dst are device buffers; m and res stay on the host.
 * Both are synchronous.                                                                      */
#define NTC_INFLATE_MAX_OUT 65536u
typedef struct ntc_inflate_member {
    uint64_t src_off;
    uint32_t src_bytes;
    uint32_t out_bytes;
    uint64_t dst_off;
} ntc_inflate_member; /* 24 bytes */
typedef struct ntc_inflate_result {
    uint32_t status, out_bytes, crc, reserved;
} ntc_inflate_result; /* 16 bytes */
int ntc_inflate_members(ntc_ctx *ctx, const uint8_t *comp, uint64_t comp_bytes, const ntc_inflate_member *m, uint64_t n,
                        uint8_t *dst, uint64_t dst_cap, ntc_inflate_result *res, uint64_t *n_failed);
int ntc_inflate_members_device(ntc_ctx *ctx, const void *d_comp, uint64_t comp_bytes, const ntc_inflate_member *m,
                               uint64_t n, void *d_dst, uint64_t dst_cap, ntc_inflate_result *res, uint64_t *n_failed);

/* ---- BGZF members of a text, made on the GPU ---------------------------------------------- */
/* A text of n bytes becomes BGZF members: gzip members with the 'B' 'C' extra field, each of at
 * most 65,280 bytes of text (NTC_BGZF_MEMBER) and at most 65,316 bytes itself, independent of
 * one another, so that bgzip, gzip and zlib read their concatenation.
 *   rec_off == NULL  the members are the consecutive 65,280-byte slices of the text.
 *   rec_off          n_rec + 1 non-decreasing offsets, rec_off[0] = 0, rec_off[n_rec] = n (else
 *                    NTC_ERR_INVALID_ARG).  cut_j is the largest offset <= 61,440 j (NTC_BGZF_GRID);
 *                    the bytes between two cuts are one member, or when they pass 65,280,
 *                    slices of 65,280.  Every member then starts and ends on a record boundary
 *                    unless a record is longer than 3,841 bytes.
 * A member is coded as two chunks (32,768 bytes, then the rest) by the coder of `--deflate gpu`
 * (ntc_deflate_stream, engine NTC_DEFLATE_GPU), so it is at most its text + 36 bytes.
 * ntc_bgzf_bound(n) = n + 36 (ceil(n / 61,440) + floor(n / 65,280)): the most bytes the rule can
 * make of n bytes whatever the offsets.  out_cap below it is NTC_ERR_CAPACITY with *out_bytes =
 * the bound, before anything is launched.  No EOF member (NTC_BGZF_EOF) is appended.
 * members (may be NULL): the table, entry i = member i's text offset, text bytes, place in out
 * and bytes there; *n_members = their number; NTC_ERR_CAPACITY when members_cap is smaller.
 *   ntc_bgzf_compress         host to host through the GPU (bgzf.hip); with ctx == NULL the host
 *                             restatement, the same rule and coder run by one lane: same bytes.
 *   ntc_bgzf_compress_device  d_text, d_rec_off and d_out are device buffers.
 * Both are synchronous; n < 4 GiB per call.
 * ntc_ctx_set_option(ctx, "bgzf_text", 1) (default 0: nothing new is launched, no byte or copy
 * changes) makes ntc_decode_fasta and ntc_decode_fasta_unpacked plan and code the formatted text
 * on the device, its records being the offsets: out then gets the members alone and *out_len
 * their bytes; the capacity to offer (and what a size query answers) is ntc_bgzf_bound(text
 * bytes) + 72.  Under "paired" each of the two parts is planned on its own and
 * ntc_decode_pair_split gives the bytes of part 1's members; a window (ntc_decode_set_window)
 * gives the members of the window's text; "discard_text" wins: nothing is compressed.
 * "bgzf_workgroups" (default 0: two per compute unit): the workgroups that share the chunks of
 * a call, a test hook.
 * ntc_bgzf_last: what the context's last call that made members left -- either call above, or
 * a text decode under "bgzf_text" -- as counts and, when members is not NULL, its table (for a
 * paired decode both parts', places as in `out`).                                              */
#define NTC_BGZF_MEMBER 65280
#define NTC_BGZF_GRID 61440
#define NTC_BGZF_EOF "\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00\x42\x43\x02\x00\x1b\x00\x03\x00\x00\x00\x00\x00\x00\x00\x00\x00"
#define NTC_BGZF_EOF_BYTES 28
typedef struct ntc_bgzf_member {
    uint64_t text_off, text_bytes, place, bytes;
} ntc_bgzf_member; /* 32 bytes */
typedef struct ntc_bgzf_counts {
    uint64_t members, text_bytes, bytes;
    uint64_t chunks_stored, chunks_huffman, chunks_matches; /* the chunks by the encoding chosen */
    double seconds; /* inside the plan, the coder and the members' copy, waiting included */
} ntc_bgzf_counts;
uint64_t ntc_bgzf_bound(uint64_t n);
int ntc_bgzf_compress(ntc_ctx *ctx, const uint8_t *text, uint64_t n, const uint64_t *rec_off, uint64_t n_rec, uint8_t *out,
                      uint64_t out_cap, ntc_bgzf_member *members, uint64_t members_cap, uint64_t *n_members, uint64_t *out_bytes);
int ntc_bgzf_compress_device(ntc_ctx *ctx, const void *d_text, uint64_t n, const uint64_t *d_rec_off, uint64_t n_rec, void *d_out,
                             uint64_t out_cap, ntc_bgzf_member *members, uint64_t members_cap, uint64_t *n_members,
                             uint64_t *out_bytes);
int ntc_bgzf_last(ntc_ctx *ctx, ntc_bgzf_counts *counts, ntc_bgzf_member *members, uint64_t members_cap, uint64_t *n_members);

/* ---- GPU unpacker (the inverse of the packer) ------------------------------------------ */
/* decode_block (src/lib.rs:320-368) split at inflate.  ntc_read_block_streams (host): one
 * block's four stream headers at data[0..len) and their gzip members inflated into
 * payload[0..capacity) (stream i at meta->stream[i].offset, 8-byte aligned, exactly
 * encoded_size words each: the big-endian words compress_block wrote); meta->n_recs = the
 * block's records (its flag stream's values), num_records its header field.  Returns what
 * ntc_read_block_into returns for a block it cannot read (NTC_ERR_IO at a clean end,
 * NTC_ERR_FORMAT damaged, NTC_ERR_CAPACITY past capacity).
 * ntc_unpack_streams (GPU): payload[0..payload_bytes) holding n_blocks blocks' streams at
 * their metas' offsets -> the blocks' u64 records in the context's device memory, in
 * block order: rice_decode / minimal_binary_decode / zip_block_contents
 * (src/decode.rs:51-149) on the device.  *n_blocks_ok = the blocks before the first
 * damaged one (a meta with status != 0, or one the device cannot decode: decode_block's
 * Err ends the reference's loop, main.rs:202); *n_reads / *n_bases = what those blocks'
 * records hold.  Synchronous.
 * ntc_unpacked_records: those records to the host (tests).  ntc_decode_fasta_unpacked:
 * ntc_decode_fasta of those records without their trip through host memory (*out_len =
 * the text's bytes; NTC_ERR_CAPACITY past out_capacity, so capacity 0 asks the size).    */
int ntc_read_block_streams(const uint8_t *data, uint64_t len, uint64_t *consumed, uint8_t *payload,
                           uint64_t capacity, ntc_block_meta *meta);
int ntc_unpack_streams(ntc_ctx *ctx, const uint8_t *payload, uint64_t payload_bytes, const ntc_block_meta *metas,
                       uint64_t n_blocks, uint64_t *n_blocks_ok, uint64_t *n_reads, uint64_t *n_bases);
int ntc_unpacked_records(ntc_ctx *ctx, uint64_t *recs, uint64_t capacity, uint64_t *n_recs);
int ntc_decode_fasta_unpacked(ntc_ctx *ctx, uint64_t first_id, uint8_t *out, uint64_t out_capacity,
                              uint64_t *out_len);

/* ---- FASTQ parsed on the GPU ------------------------------------------------------------ */
/* The CLI's ingest (src/main.rs:158-163: needletail records + normalize(true)) for plain
 * FASTQ, done on the device: fastq[0, fastq_bytes) is the text of exactly n_reads records of
 * 4 lines each ('@' header, sequence, '+' line, quality as long as the sequence after one
 * '\r' is stripped from each; the last line may lack its newline) and nothing else -- no
 * blank lines, which the host parser (ntc_fastx_*) skips between records and the caller
 * sends there.  Bases are the sequence lines normalised as ntc_fastx does.  Text under
 * 4 GiB per call.  NTC_ERR_FORMAT (bad_read = the first failing record) if the text is not
 * that.  Synchronous; fastq should be pinned host memory for full PCIe speed.
 *   ntc_fastq_parse        bases + read_offsets[n_reads + 1] back to the host (tests, tools);
 *                          *n_bases = bases parsed (NTC_ERR_CAPACITY past bases_capacity)
 *   ntc_encode_pack_fastq  ntc_encode_pack_batch on the parsed reads, which never leave
 *                          HBM: same metas and payload as parsing on the host and calling
 *                          ntc_encode_pack_batch; *n_bases = bases encoded              */
int ntc_fastq_parse(ntc_ctx *ctx, const uint8_t *fastq, uint64_t fastq_bytes, uint64_t n_reads, uint8_t *bases_out,
                    uint64_t bases_capacity, uint64_t *read_offsets_out, uint64_t *n_bases, int64_t *bad_read);
int ntc_encode_pack_fastq(ntc_ctx *ctx, const uint8_t *fastq, uint64_t fastq_bytes, uint64_t n_reads,
                          uint32_t block_reads, ntc_block_meta *meta, uint8_t **payload, uint64_t *payload_bytes,
                          uint64_t *n_bases, int64_t *bad_read);

/* ---- exception side file ("NTCX", version 1) ---------------------------------------------- */
/* The exception runs of an encoded.dat written under policy keep (ntcomp_gpu.h, "non-ACGT
 * symbols"), beside it and never inside it.  Everything little-endian:
 *   header, 32 bytes: "NTCX", u32 version = 1, u8 sub (the substitute base), 23 zero bytes
 *   sections until the end of the file: u64 n_runs, u64 0, then n_runs runs of 24 bytes
 *     (ntc_nx_run: u64 read, u32 pos, u32 len, u32 sym, u32 0)
 * `read` counts the reads of the blocks that were written: N - 1 of the ">seq.N" line decode
 * prints (a block the pipeline drops takes its runs with it, and later reads move down).
 * Across the whole file the runs increase strictly by (read, pos) and do not overlap.  A file
 * without runs is the header alone.
 * ntc_nx_write (host): the header when with_header, then one section of n_runs runs when
 * n_runs > 0, to fd.  NTC_ERR_IO on a short write, NTC_ERR_INVALID_ARG for a sub other than
 * A/C/G/T.
 * ntc_nx_read (host): parses and validates the file at path; *runs (all sections, in file
 * order; free with ntc_buffer_free; null when there are none), *n_runs, *sub.  NTC_ERR_IO if
 * it cannot be read; NTC_ERR_FORMAT for a bad magic or version, a truncated header, section
 * or run, a non-zero pad, len = 0, pos + len past 2^32, a sym that is not one of the twelve
 * symbols, runs out of order or overlapping, a sub that is not A/C/G/T.                      */
int ntc_nx_write(int fd, const ntc_nx_run *runs, uint64_t n_runs, uint32_t sub, int with_header);
int ntc_nx_read(const char *path, ntc_nx_run **runs, uint64_t *n_runs, uint32_t *sub);

/* ---- FASTQ quality scores ------------------------------------------------------------------ */
/* ntc_ctx_set_option(ctx, "qualities", mode) says what ntc_encode_pack_fastq does with the
 * quality lines of its text:
 *   0  drop (default): they are skipped, as ever; neither their length against the bases kept
 *      nor their bytes are checked.
 *   1  keep (lossless): every block of block_reads reads also yields a quality section.
 *   2  bin8 (lossy): Phred q = byte - 33 is first mapped to 8 levels (q < 2 stays, 2-9 -> 6,
 *      10-19 -> 15, 20-24 -> 22, 25-29 -> 27, 30-34 -> 33, 35-39 -> 37, >= 40 -> 40), then as 1.
 * A read's qualities are its quality line without one trailing '\r'; under 1 and 2 their
 * number must equal the read's bases after normalisation and every byte must lie in '!'..'~',
 * else the call returns NTC_ERR_FORMAT with that read as bad_read.  The calls that take bases
 * without qualities (ntc_encode_batch, ntc_encode_batch_device, ntc_encode_pack_batch) return
 * NTC_ERR_UNSUPPORTED under 1 and 2.
 *
 * A section, the canonical packed form of one block: alphabet = the distinct quality bytes of
 * the block, ascending (n_syms of them, 1..94); width = 0, 1, 2, 4 or 8 bits for n_syms = 1,
 * 2, 3-4, 5-16, more; quality i of the block (read by read) has the rank of its byte in the
 * alphabet as its code, in bits [i width, i width + width) of a little-endian bit stream of
 * ceil(n_quals width / 64) 64-bit words, unused high bits zero.  The packing runs on the GPU.
 *
 * ntc_ctx_set_option(ctx, "quality_coder", c) chooses the sections' coder: 0 pack (default, the
 * form above), 1 rans.  The option holds until it is changed, can be read with
 * ntc_ctx_get_option, and is ignored under qualities = 0.  Under 1 a section is coded on the
 * GPU by a static order-1 rANS coder; its meta has reserved[0] = 1, width still follows from
 * n_syms, payload_off is 8-aligned, payload_bytes is exact, and the body there is canonical
 * (one input, one byte string):
 *   symbols   a quality's symbol is its rank in the alphabet; the block's qualities are cut into
 *             spans of 2048, whatever the reads, the last one may be shorter
 *   context   the symbol before it in the same span; n_syms at a span's start: n_syms + 1 rows
 *   table     (n_syms + 1) * n_syms u16, row-major: counts over the whole block per (context,
 *             symbol), each row normalised to sum 4096: f = 0 where the count is 0, else
 *             max(1, floor(c * 4096 / T)); the difference to 4096 goes to the symbol with the
 *             largest count (lowest index on ties); a row never seen is all zeros
 *   sizes     ceil(n_quals / 2048) u32: the bytes of each span's stream
 *   streams   back to back.  Byte-wise rANS, 32-bit state, L = 2^23: the encoder starts at L
 *             and takes the span's symbols last to first; for start c (the frequencies below
 *             the symbol in its row) and frequency f: while x >= 2^19 f emit x & 0xFF and shift
 *             x >>= 8, then x = ((x / f) << 12) + x % f + c.  The stream is the final state as
 *             u32, then the emitted bytes in reverse order.  The decoder reads forward: x = the
 *             first 4 bytes; per symbol slot = x & 4095, s the symbol with c_s <= slot < c_s +
 *             f_s, x = f_s (x >> 12) + slot - c_s, and while x < L: x = x << 8 | next byte.  At
 *             the end x = L and the span's bytes are used up.
 * A section with n_syms <= 1 has an empty body.
 *
 * Smoothing inside long matches (lossy), three more options of the context:
 *   "quality_smooth"     0 (off, default) or M in 12..16777215
 *   "quality_smooth_to"  the target T, a byte in '$'..'~' (default 'I')
 *   "quality_smoothed"   read-only: the bytes the last ntc_encode_pack_fastq call replaced
 *                        ("quality_smoothed_total": of all calls since quality_smooth was set)
 * A read's records come in archive order, rightmost first, with lengths L_0 .. L_{m-1}; record j
 * covers positions [e_j - L_j, e_j) of the read, e_0 = its bases, e_{j+1} = e_j - L_j.  A
 * position is trusted iff it lies in a long record (flag bit 1 of byte 7 clear) with L_j >= M.
 * With tab the mode's table: a byte q = tab[input] at a trusted position with q > tab['#']
 * becomes tab[T]; every other byte stays (scores at or below the image of '#' are the no-call
 * marker, which is never raised).  The pass runs on the GPU once the call has its final
 * records, and everything after it sees the smoothed bytes: the alphabets and widths, the
 * packed words, the rANS tables and streams, and the qual digest (which is that of the bytes
 * decode prints).  The records, the packed blocks, every other side list and the section
 * format are those of a call without it.  ntc_encode_pack_fastq returns NTC_ERR_INVALID_ARG
 * when M is set under qualities = 0, or when tab[T] <= tab['#'] (under mode 2, T in '$'..'*').
 * The options hold until they are changed. */
typedef struct ntc_qual_meta {
    uint64_t n_reads;       /* reads of the block                                          */
    uint64_t n_quals;       /* their quality bytes (= their bases)                         */
    uint64_t payload_off;   /* byte offset of the section's words in the payload buffer    */
    uint64_t payload_bytes; /* 8 * ceil(n_quals * width / 64); coder 1: the body's bytes   */
    uint8_t width, n_syms;
    uint8_t reserved[6];    /* [0]: the coder, 0 pack, 1 rans; the rest 0                  */
    uint8_t alphabet[96];   /* n_syms bytes ascending, then zeros                          */
} ntc_qual_meta;            /* 136 bytes */
/* The sections of the last ntc_encode_pack_fastq call on this context under mode 1 or 2, one
 * per block (none under mode 0, or when that call failed): metas[0 .. *n_blocks) and their
 * words in payload, *payload_bytes in all.  NTC_ERR_CAPACITY (sizes set, nothing copied) when
 * meta_cap or payload_cap is smaller.                                                      */
int ntc_encode_qualities(ntc_ctx *ctx, ntc_qual_meta *metas, uint64_t meta_cap, uint8_t *payload,
                         uint64_t payload_cap, uint64_t *n_blocks, uint64_t *payload_bytes);
/* Sections (copied) for the next ntc_decode_fasta or ntc_decode_fasta_unpacked call on this
 * context: section i covers the next metas[i].n_reads reads of that call, which then writes
 * FASTQ -- "@seq.{id}\n{read}\n+\n{qualities}\n" -- instead of FASTA, and returns
 * NTC_ERR_FORMAT (no text) when the sections do not cover exactly its reads, a block's
 * n_quals differs from the bases decoded for its reads, or a code is >= n_syms.  Checked here,
 * NTC_ERR_FORMAT: each width against n_syms, an ascending alphabet within '!'..'~',
 * payload_bytes of every section, and that it lies 8-byte aligned inside the payload.  The
 * sections are dropped by the call that used them, whatever it returned (a call that only
 * reports sizes keeps them); ntc_decode_batch and ntc_decode_batch_device ignore them.
 * n_blocks = 0 drops pending sections.
 * Sections of coder 1 (all of them, or none) are decoded on the GPU.  Checked here for them,
 * NTC_ERR_FORMAT: every row of the table sums to 4096 or is all zero, the start row is not zero
 * when n_quals > 0, the span sizes number ceil(n_quals / 2048), each is >= 4 and they sum to the
 * rest of the body, and the body is empty exactly when n_syms <= 1.  The decode call returns
 * NTC_ERR_FORMAT (no text) also for a slot that falls in no symbol of its row, a byte needed
 * past a span's end, a final state other than L and bytes of a span left over.               */
int ntc_decode_set_qualities(ntc_ctx *ctx, const ntc_qual_meta *metas, uint64_t n_blocks, const uint8_t *payload,
                             uint64_t payload_bytes);

/* ---- quality side file ("NTCQ", versions 1 and 2) ------------------------------------------- */
/* The quality sections of an encoded.dat, beside it.  Everything little-endian:
 *   header, 32 bytes: "NTCQ", u32 version = 1, u8 mode (1 keep, 2 bin8), 23 zero bytes
 *   sections until the end of the file, section i for block i of encoded.dat:
 *     24 bytes: u64 n_reads, u64 n_quals, u8 width, u8 n_syms, u16 0, u32 gz_bytes
 *     n_syms alphabet bytes
 *     one gzip member of gz_bytes bytes holding the section's words (gz_bytes = 0 at width 0)
 * ntc_q_write_header / ntc_q_write_section (host) write them to fd; ntc_q_deflate_section
 * returns a section's bytes (free with ntc_buffer_free) so that a thread pool can make them.
 * words = the section's payload_bytes bytes; engine as for ntc_deflate_block.  NTC_ERR_IO on a
 * short write, NTC_ERR_INVALID_ARG for a meta that is not canonical.
 * ntc_q_read (host) parses and validates the file at path: *metas (payload_off into *payload;
 * both freed with ntc_buffer_free, null when empty), *mode.  NTC_ERR_IO if it cannot be read;
 * NTC_ERR_FORMAT for a bad magic, version or mode, a truncated header, alphabet or member, a
 * width that does not follow from n_syms, an alphabet that is not ascending or leaves
 * '!'..'~', a member that does not inflate to exactly payload_bytes, non-zero padding bits.
 *
 * Version 2 holds sections of coder 1 (rans); files of coder 0 are always version 1:
 *   header, 32 bytes: "NTCQ", u32 version = 2, u8 mode, u8 coder = 1, 22 zero bytes
 *   sections as above, the last header field being the body's bytes; after the alphabet comes
 *   the body as it is, no gzip member
 * ntc_q_write_header2 writes the header of a coder (0: the version-1 header).  For a meta with
 * reserved[0] = 1, ntc_q_deflate_section and ntc_q_write_section emit a version-2 section
 * (engine is ignored; NTC_ERR_INVALID_ARG for a body ntc_decode_set_qualities would refuse).
 * ntc_q_read reads both versions; for version 2 every body starts 8-aligned in *payload, and
 * NTC_ERR_FORMAT is also a coder byte other than 1 and everything ntc_decode_set_qualities
 * checks of a body.                                                                          */
int ntc_q_write_header(int fd, int mode);
int ntc_q_write_header2(int fd, int mode, int coder);
int ntc_q_deflate_section(const ntc_qual_meta *meta, const uint8_t *words, int engine, uint8_t **out,
                          uint64_t *out_len);
int ntc_q_write_section(int fd, const ntc_qual_meta *meta, const uint8_t *words, int engine);
int ntc_q_read(const char *path, int *mode, ntc_qual_meta **metas, uint64_t *n_blocks, uint8_t **payload,
               uint64_t *payload_bytes);

/* ---- FASTQ read names ----------------------------------------------------------------------- */
/* ntc_ctx_set_option(ctx, "names", mode) says what ntc_encode_pack_fastq does with the header
 * lines of its text:
 *   0  drop (default): only their '@' is looked at, as ever.
 *   1  keep (lossless): every block of block_reads reads also yields a name section.
 *   2  id (lossy): each name is first cut before its first space or tab, then as 1.
 * A read's name is its header line without the '@' and without one trailing '\r'.  It may be
 * empty and may hold any byte but '\n'; after the cut it is at most NTC_NAME_MAX bytes, else
 * the call returns NTC_ERR_FORMAT with the lowest such read as bad_read.  The calls that take
 * bases without header lines (ntc_encode_batch, ntc_encode_batch_device,
 * ntc_encode_pack_batch) return NTC_ERR_UNSUPPORTED under 1 and 2.
 *
 * A section, the canonical front- and back-coded form of one block's names.  The chain
 * restarts every NTC_NAME_GROUP reads of the block.  With P the name of read i - 1 and N that
 * of read i: pre_i = suf_i = 0 when i % NTC_NAME_GROUP == 0, else pre_i = min(255, lcp(P, N))
 * and suf_i = min(255, longest common suffix, |P| - pre_i, |N| - pre_i); mid_i = N[pre_i :
 * |N| - suf_i].  Payload: len[n] as little-endian u16, pre[n] as u8, suf[n] as u8, the mids
 * in read order, zero bytes up to a multiple of 8.  Decoding: N = P[:pre] + mid + P[|P| -
 * suf:], valid iff pre + suf <= min(len_i, len_{i-1}).  The coding runs on the GPU.          */
#define NTC_NAME_MAX 4095
#define NTC_NAME_GROUP 64
typedef struct ntc_name_meta {
    uint64_t n_reads;       /* reads of the block                                          */
    uint64_t name_bytes;    /* sum of len                                                  */
    uint64_t mid_bytes;     /* sum of the mids                                             */
    uint64_t payload_off;   /* byte offset of the section in the payload buffer            */
    uint64_t payload_bytes; /* 8 * ceil((4 n_reads + mid_bytes) / 8)                       */
} ntc_name_meta;            /* 40 bytes */
/* The sections of the last ntc_encode_pack_fastq call on this context under mode 1 or 2, one
 * per block (none under mode 0, or when that call failed); capacities as for
 * ntc_encode_qualities.                                                                     */
int ntc_encode_names(ntc_ctx *ctx, ntc_name_meta *metas, uint64_t meta_cap, uint8_t *payload, uint64_t payload_cap,
                     uint64_t *n_blocks, uint64_t *payload_bytes);
/* Sections (copied) for the next ntc_decode_fasta or ntc_decode_fasta_unpacked call on this
 * context: section i covers the next metas[i].n_reads reads of that call, which then writes
 * ">{name}\n{read}\n" (or "@{name}\n{read}\n+\n{qualities}\n" when quality sections are
 * pending too) instead of seq.N, and returns NTC_ERR_FORMAT (no text) when the sections do
 * not cover exactly its reads or a section breaks a rule above (a len past NTC_NAME_MAX, pre
 * + suf past either neighbour, pre or suf on a restart read, mids or names that do not sum to
 * the meta).  Checked here, NTC_ERR_FORMAT: payload_bytes of every section against n_reads
 * and mid_bytes, and that it lies 8-byte aligned inside the payload.  The sections are
 * dropped by the call that used them, whatever it returned (a call that only reports sizes
 * keeps them); ntc_decode_batch and ntc_decode_batch_device ignore them.  n_blocks = 0 drops
 * pending sections.                                                                         */
int ntc_decode_set_names(ntc_ctx *ctx, const ntc_name_meta *metas, uint64_t n_blocks, const uint8_t *payload,
                         uint64_t payload_bytes);

/* ---- name side file ("NTCN", version 1) ----------------------------------------------------- */
/* The name sections of an encoded.dat, beside it.  Everything little-endian:
 *   header, 32 bytes: "NTCN", u32 version = 1, u8 mode (1 keep, 2 id), 23 zero bytes
 *   sections until the end of the file, section i for block i of encoded.dat:
 *     32 bytes: u64 n_reads, u64 name_bytes, u64 mid_bytes, u32 gz_bytes, u32 0
 *     one gzip member of gz_bytes bytes that inflates to exactly the section's payload_bytes
 * The functions mirror the quality file's.  ntc_n_deflate_section / ntc_n_write_section:
 * NTC_ERR_INVALID_ARG for a meta that is not canonical (payload_bytes, mid_bytes against
 * name_bytes, name_bytes against n_reads).  ntc_n_read validates everything: NTC_ERR_FORMAT
 * for a bad magic, version or mode, truncation, a non-zero pad word, a member that does not
 * inflate to exactly payload_bytes, a len past NTC_NAME_MAX, pre + suf past either
 * neighbour, a restart read with pre or suf, mids that do not sum to mid_bytes, names that
 * do not sum to name_bytes, non-zero padding bytes.                                         */
int ntc_n_write_header(int fd, int mode);
int ntc_n_deflate_section(const ntc_name_meta *meta, const uint8_t *payload, int engine, uint8_t **out,
                          uint64_t *out_len);
int ntc_n_write_section(int fd, const ntc_name_meta *meta, const uint8_t *payload, int engine);
int ntc_n_read(const char *path, int *mode, ntc_name_meta **metas, uint64_t *n_blocks, uint8_t **payload,
               uint64_t *payload_bytes);

/* ---- per-block content digests -------------------------------------------------------------- */
/* ntc_ctx_set_option(ctx, "digests", 1) (default 0: nothing is launched) makes
 * ntc_encode_pack_fastq and ntc_encode_pack_batch also digest, on the GPU, what each block of
 * block_reads reads holds, so that a decode can check that it gave the same bytes back.  All
 * arithmetic is modulo 2^64:
 *   mix(x):  x ^= x >> 30;  x *= 0xBF58476D1CE4E5B9;  x ^= x >> 27;  x *= 0x94D049BB133111EB;
 *            x ^= x >> 31
 *   K0 = 0xD6E8FEB86659FD93, K1 = 0x9E3779B97F4A7C15
 *   h(s), s a string of n bytes:  w_j = the little-endian u64 of s[8j .. 8j + 8), zero-padded
 *            past n;  h(s) = mix((n + 1) K0 + sum_j mix(w_j + (j + 1) K1))
 *   D(s_0 .. s_{m-1}) = sum_i mix(h(s_i) + (i + 1) K1),  i = the read's index inside the block
 * It guards against accident (another index, a damaged or truncated file, an unmatched side
 * file), not against an adversary.  A block has one D per component; s_i is
 *   NTC_DIGEST_SEQ   the read's bases as the records hold them: after the non-ACGT pass has put
 *                    in the substitute base.  Always present.
 *   NTC_DIGEST_SYM   the read's symbols before that pass.  Present under non_acgt 2 (keep).
 *   NTC_DIGEST_QUAL  the quality bytes as a decode prints them (after bin8's mapping).  Present
 *                    under qualities 1 and 2 (ntc_encode_pack_fastq only).
 *   NTC_DIGEST_NAME  the name as a decode prints it (after id's cut).  Present under names 1 and
 *                    2 (ntc_encode_pack_fastq only).                                          */
#define NTC_DIGEST_SEQ 1u
#define NTC_DIGEST_SYM 2u
#define NTC_DIGEST_QUAL 4u
#define NTC_DIGEST_NAME 8u
typedef struct ntc_digest_meta {
    uint64_t n_reads;    /* reads of the block                                             */
    uint64_t n_bases;    /* their bases                                                    */
    uint64_t d_seq;      /* the component digests; 0 for a component that is not present   */
    uint64_t d_sym;
    uint64_t d_qual;
    uint64_t d_name;
    uint32_t components; /* NTC_DIGEST_* bits: present (encode, expected) / checked (decode) */
    uint32_t reserved;   /* 0                                                              */
} ntc_digest_meta;       /* 56 bytes */
/* The digests of the last ntc_encode_pack_fastq or ntc_encode_pack_batch call on this context
 * with "digests" 1, one entry per block (none with "digests" 0, or when that call failed).
 * *n_blocks = their number; NTC_ERR_CAPACITY (nothing copied) when cap is smaller.          */
int ntc_encode_digests(ntc_ctx *ctx, ntc_digest_meta *metas, uint64_t cap, uint64_t *n_blocks);
/* Expected digests (copied) for the next ntc_decode_fasta or ntc_decode_fasta_unpacked call on
 * this context: entry i covers the next metas[i].n_reads reads of that call, which digests on
 * the GPU what it decoded -- seq right after the walk, sym after the exception runs went in
 * (only when runs were pending), qual and name after their sections were expanded (only when
 * those were pending) -- and compares there every component it could compute whose bit the
 * entry has.  A block whose bases count or digest differs makes the call return
 * NTC_ERR_DIGEST and write no text; ntc_last_error names the block, the component and both
 * values.  NTC_ERR_FORMAT when the entries do not cover exactly the call's reads.  Checked
 * here, NTC_ERR_INVALID_ARG: a bit outside NTC_DIGEST_*, a missing NTC_DIGEST_SEQ, a non-zero
 * digest of an absent component, reserved != 0.  The entries are dropped by the call that
 * used them, whatever it returned (a call that only reports sizes keeps them);
 * ntc_decode_batch and ntc_decode_batch_device ignore them.  n_blocks = 0 drops them.      */
int ntc_decode_set_digests(ntc_ctx *ctx, const ntc_digest_meta *metas, uint64_t n_blocks);
/* What the last ntc_decode_fasta / ntc_decode_fasta_unpacked call that was given expected
 * digests computed, also after NTC_ERR_DIGEST: entry i has that block's reads, bases and the
 * digests of the components it could check (components says which; the others are 0).
 * Capacity protocol as above.
 * A verification pass needs no text: with ntc_ctx_set_option(ctx, "discard_text", 1) (default
 * 0) ntc_decode_fasta and ntc_decode_fasta_unpacked run as ever, the formatter included, but do
 * not copy the text to the host; out may then be NULL and out_capacity 0, and *out_len is
 * still the text's size.                                                                    */
int ntc_decode_digests(ntc_ctx *ctx, ntc_digest_meta *metas, uint64_t cap, uint64_t *n_blocks);

/* ---- digest side file ("NTCD", version 1) --------------------------------------------------- */
/* The digests of an encoded.dat, beside it.  Everything little-endian, nothing deflated:
 *   header, 32 bytes: "NTCD", u32 version = 1, u8 components (the union over the file), 3 zero
 *     bytes, u32 k and u64 n_nodes of the index it was written against (ntc_index_info), 8 zero
 *     bytes
 *   one 56-byte ntc_digest_meta per block of encoded.dat, until the end of the file
 * ntc_d_read refuses with NTC_ERR_FORMAT: a bad magic or version, non-zero padding, a length
 * that is not 32 + 56 m, a component bit outside the header's (or a header without
 * NTC_DIGEST_SEQ, or a section without it), a non-zero digest of an absent component.
 * ntc_d_write_header / ntc_d_write_section refuse the same with NTC_ERR_INVALID_ARG (a
 * section is checked against NTC_DIGEST_* alone; its reader checks it against the header).
 * *metas is malloc'ed (free() it; NULL when there is no section).                           */
int ntc_d_write_header(int fd, uint32_t components, uint32_t k, uint64_t n_nodes);
int ntc_d_write_section(int fd, const ntc_digest_meta *meta);
int ntc_d_read(const char *path, uint32_t *components, uint32_t *k, uint64_t *n_nodes, ntc_digest_meta **metas,
               uint64_t *n_blocks);

/* ---- paired-end reads ------------------------------------------------------------------------ */
/* A paired archive is an ordinary one whose reads alternate: read 2p is mate 1 of pair p, read
 * 2p + 1 its mate 2.  No format changes and nothing records it: the caller says so, here as at
 * decode.  ntc_ctx_set_option(ctx, "paired", v): 0 off (default: nothing below is launched),
 * 1 pairs with the mate check, 2 pairs without it; anything else NTC_ERR_INVALID_ARG.
 *
 * The mate rule (check 1): id(N) = the name N cut before its first space or tab; with a =
 * id(name of read 2p) and b = id(name of read 2p + 1), when a ends in "/1" and b ends in "/2"
 * both lose those two bytes; the mates agree iff a == b byte for byte.  (Two empty names
 * agree; "x/1" beside "x" and "x/2" beside "x/1" do not.)
 *
 * Under 1 and 2:
 *   ntc_encode_pack_fastq takes its text as interleaved pairs: n_reads and block_reads must be
 *     even (NTC_ERR_INVALID_ARG).  Under 1 the lowest pair whose mates disagree fails the call
 *     with NTC_ERR_FORMAT, bad_read = 2p, before anything is encoded; a failed call leaves no
 *     sections.
 *   ntc_encode_pack_fastq_paired takes the mates as two texts of n_pairs records each, weaves
 *     them on the GPU (record p of text 1, then record p of text 2; a last line without its
 *     newline gets one; line ends are otherwise copied as they are) and does what
 *     ntc_encode_pack_fastq does for 2 n_pairs reads: same metas, payload and sections as that
 *     call on the interleaved text.  NTC_ERR_INVALID_ARG under "paired" 0; NTC_ERR_CAPACITY,
 *     before anything is read, unless bytes1 + bytes2 + 2 < 4 GiB; NTC_ERR_FORMAT, before
 *     anything is woven or encoded, when a text does not hold exactly 4 n_pairs lines (a last
 *     line without its newline counts as one).
 *   ntc_decode_fasta and ntc_decode_fasta_unpacked return the text split: all mate-1 records
 *     in order, then all mate-2 records.  *out_len and the capacity protocol are unchanged (the
 *     size is the total); an odd read count is NTC_ERR_FORMAT.  Without names the reads keep
 *     the archive's numbering (seq.1, seq.3, ... in part 1).  Under "discard_text" nothing is
 *     split.  ntc_decode_pair_split: *first_bytes = the bytes of part 1 of the last such call
 *     (0 when it failed); NTC_ERR_INVALID_ARG when the last text decode was not a paired one.
 * The calls that carry neither names nor text (ntc_encode_pack_batch, ntc_encode_batch*,
 * ntc_decode_batch*) ignore the option.                                                       */
int ntc_encode_pack_fastq_paired(ntc_ctx *ctx, const uint8_t *fastq1, uint64_t bytes1, const uint8_t *fastq2,
                                 uint64_t bytes2, uint64_t n_pairs, uint32_t block_reads, ntc_block_meta *meta,
                                 uint8_t **payload, uint64_t *payload_bytes, uint64_t *n_bases, int64_t *bad_read);
int ntc_decode_pair_split(ntc_ctx *ctx, uint64_t *first_bytes);

/* ---- a window on a batch's text ---------------------------------------------------------------- */
/* ntc_decode_set_window: the next ntc_decode_fasta or ntc_decode_fasta_unpacked call on this
 * context decodes its batch whole -- walk, exception runs, qualities, names, digests: a digest
 * that differs outside the window still fails the call -- and formats only reads
 * [first, first + count) of it.  Read r of the batch keeps the id first_id + r, its name and
 * its quality line.  The window is dropped by the call that used it, whatever it returned (a
 * call that only reports sizes keeps it).  count = 0 is NTC_ERR_INVALID_ARG and drops a pending
 * window.  In the call that takes it: first + count > the batch's reads is
 * NTC_ERR_INVALID_ARG; under "paired" both numbers must be even (whole pairs), else
 * NTC_ERR_INVALID_ARG, and the split is that of the window's pairs.  out_capacity must hold the
 * whole batch's text, as a size query reports it (the window's bytes depend on each read's
 * bases and name and are only known on the device); the call copies the window's bytes alone
 * and *out_len, and ntc_decode_pair_split, report those.                                       */
int ntc_decode_set_window(ntc_ctx *ctx, uint64_t first, uint64_t count);

#ifdef __cplusplus
}
#endif
#endif
