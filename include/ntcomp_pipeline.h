/*
 * ntcomp_pipeline.h -- the CLI's native file-to-file drivers (libntcomp_gpu.so).
 *
 *   ntc_encode_file   src/main.rs:141-181 (`ntcomp encode -i P reads > encoded.dat`):
 *                     FASTX batches -> GPU encode + block packer on every context ->
 *                     deflate on the host pool -> file header + blocks, in file order.
 *                     A plain FASTQ goes to the GPU as text, cut at block boundaries,
 *                     and is parsed there (ntc_encode_pack_fastq); a batch with a blank
 *                     line, and every compressed or FASTA input, is parsed on the host.
 *   ntc_decode_file   src/main.rs:183-211 (`ntcomp decode -i P encoded.dat > out.fasta`):
 *                     blocks inflated + stream-decoded on the host pool -> GPU walk and
 *                     FASTA formatting on every context -> ">seq.N" records in file order.
 *
 * Behaviour kept from the reference: blocks of 65,536 reads (main.rs:152), the last block's
 * header carries num_records % 65,536 (main.rs:176), a block with no long or no short
 * record is not written (write_block_to errs and main.rs:170 drops it).
 * Errors are status codes (the reference panics or, for bases absent from the index, never
 * terminates): the first failing read's file index is in stats->bad_read.
 */
#ifndef NTCOMP_PIPELINE_H
#define NTCOMP_PIPELINE_H

#include <stdint.h>

#include "ntcomp_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ntc_pipeline_opts {
    int32_t threads;          /* host pool (parse, deflate); <= 0: ntc_host_threads()        */
    int32_t blocks_per_batch; /* 65,536-read blocks per GPU call; <= 0: 4 (encode), 2 (decode) */
    uint64_t batch_bases;     /* encode: bases per pinned batch buffer; 0: 64 Mi (grows for long reads) */
    int32_t deflate_engine;   /* NTC_DEFLATE_ZLIB (0), _LIBDEFLATE (1), _ADAPTIVE (2) or _GPU
                                 (3: the contexts deflate the block streams behind their packer,
                                 option "gpu_deflate"; the host writes stream headers and copies
                                 members; side sections go to the pool under _ADAPTIVE, or _ZLIB
                                 without libdeflate; NTC_ERR_UNSUPPORTED in a build without the
                                 GPU hooks).  Encode only: decode ignores the field            */
    int32_t host_parse;       /* encode, plain FASTQ: 0 = the text goes to the GPU, which parses
                                 it (ntc_encode_pack_fastq); 1 = parsed by the host pool      */
} ntc_pipeline_opts;

typedef struct ntc_pipeline_stats {
    uint64_t reads, bases, blocks, dropped_blocks, bytes_out;
    double parse_s, gpu_s, deflate_s, write_s; /* thread-seconds per stage                  */
    double wall_s;
    double alloc_s;                            /* seconds spent pinning host buffers        */
    double first_batch_s, reader_done_s, gpu_done_s; /* timeline from the call's start       */
    int32_t threads;
    int32_t gpu_parsed;                        /* encode: batches parsed on the GPU (FASTQ text) */
    int64_t bad_read;                          /* file index of the failing read, or -1     */
    char error[256];
} ntc_pipeline_stats;

/* ctxs: n_ctx contexts with the index uploaded (one per GPU; two on one device are allowed).
 * Writes encoded.dat to out_fd (not closed).                                              */
int ntc_encode_file(ntc_ctx *const *ctxs, int n_ctx, const char *in_path, int out_fd, const ntc_pipeline_opts *opts,
                    ntc_pipeline_stats *stats);

/* Reads encoded.dat at in_path (mapped), writes FASTA to out_fd (not closed): ">seq.i\n"
 * + bases + "\n" per read, i from 1 across the file (main.rs:204).  opts->threads sizes the
 * inflate pool, opts->blocks_per_batch the GPU call (<= 0: 2; batch_bases and
 * deflate_engine are unused).  A truncated block ends the input like read_exact (main.rs:199); a damaged block
 * (bad gzip member or stream sizes) ends the output after the blocks before it and still
 * returns NTC_OK, as decode_block's Err just ends the reference's loop (main.rs:202): the
 * caller sees it in stats->dropped_blocks (> 0) and stats->error.  stats: reads, bases,
 * blocks decoded, dropped_blocks = whole blocks not decoded, bytes_out = FASTA bytes,
 * parse_s = inflate CPU time summed over threads, gpu_s, write_s, wall_s, alloc_s = block
 * scan + pinned allocation seconds, first_batch_s / reader_done_s / gpu_done_s = when the
 * first batch was written / the last block inflated / the last GPU call returned.            */
int ntc_decode_file(ntc_ctx *const *ctxs, int n_ctx, const char *in_path, int out_fd, const ntc_pipeline_opts *opts,
                    ntc_pipeline_stats *stats);

/* ---- reads with N and IUPAC symbols ------------------------------------------------------- */
/* ntc_encode_file under a non-ACGT policy (ntcomp_gpu.h): NTC_NX_ERROR = ntc_encode_file;
 * NTC_NX_MASK replaces each such symbol by the substitute base (lossy); NTC_NX_KEEP also
 * writes the replaced symbols as exception runs to nx_fd (not closed), in the "NTCX" format
 * of ntcomp_codec.h -- always, so a file without such symbols gets the header alone.  nx_fd
 * must be >= 0 under NTC_NX_KEEP and -1 otherwise (NTC_ERR_INVALID_ARG).  encoded.dat has
 * the reference's layout under every policy; decoded without the side file it gives the
 * masked reads.  The contexts' "non_acgt" option is set for the call and left at 0.
 * A run's `read` counts the reads of the blocks written: a block the pipeline drops (no long
 * or no short record, App. B.3) takes its runs with it and later reads move down, exactly
 * as decode numbers its ">seq.N" lines.
 * nx (may be NULL): runs = runs written to the side file (NTC_NX_MASK: runs found), bases =
 * symbols replaced (dropped blocks included), reads = reads with a run in the side file
 * (NTC_NX_MASK: 0), runs_in_dropped_blocks = runs not written because their block was
 * dropped (NTC_NX_MASK: 0).
 * ntc_decode_file_nx: ntc_decode_file, with the side file at nx_path (NULL: none) read once
 * (ntc_nx_read) and each batch's runs put back before its text is formatted.  A side file
 * that does not belong to this encoding -- a run past a read's end or over a base that is
 * not the recorded substitute -- is NTC_ERR_FORMAT.                                        */
enum { NTC_NX_ERROR = 0, NTC_NX_MASK = 1, NTC_NX_KEEP = 2 };
typedef struct ntc_nx_stats {
    uint64_t runs, bases, reads, runs_in_dropped_blocks;
} ntc_nx_stats;
int ntc_encode_file_nx(ntc_ctx *const *ctxs, int n_ctx, const char *in_path, int out_fd, int policy, int nx_fd,
                       const ntc_pipeline_opts *opts, ntc_pipeline_stats *stats, ntc_nx_stats *nx);
int ntc_decode_file_nx(ntc_ctx *const *ctxs, int n_ctx, const char *in_path, const char *nx_path, int out_fd,
                       const ntc_pipeline_opts *opts, ntc_pipeline_stats *stats);

/* ---- both side files: exceptions and quality scores ----------------------------------------- */
/* ntc_encode_file_ex / ntc_decode_file_ex take both side files in one options struct, so that
 * --non-acgt keep and --qualities keep work together.
 * Encode: nx_policy / nx_fd as ntc_encode_file_nx takes them.  q_mode 0 (drop): no quality
 * file, q_fd must be -1.  q_mode 1 (keep) or 2 (bin8, ntcomp_codec.h): every block written to
 * encoded.dat gets its quality section in the "NTCQ" file at q_fd (>= 0, not closed), packed
 * on the GPU and deflated by the pipeline's pool with the block's streams; a block the
 * pipeline drops takes its section with it.  encoded.dat is byte for byte that of a run
 * without qualities, and the side file does not depend on the number of contexts or on
 * whether the same text came plain or compressed.  Qualities exist only where the GPU parses
 * the FASTQ text: host_parse = 1, an input that is not FASTQ, and a batch that falls back to
 * the host parser (a blank line) are NTC_ERR_UNSUPPORTED under modes 1 and 2, with the case
 * in stats->error.  The contexts' "qualities" option is set for the call and left at 0.
 * q (may be NULL): sections and qualities written, their packed and deflated bytes.
 * The sections' coder is the contexts' "quality_coder" option (ntcomp_codec.h: 0 pack, 1 rans),
 * which the call leaves as it is; contexts that disagree are NTC_ERR_INVALID_ARG.  Under 1 the
 * file is version 2, the pool copies each section's body as it came off the device instead of
 * deflating it, and every property above holds as well; q->packed_bytes is then the bodies'
 * bytes and q->deflated_bytes the sections' bytes as written.  Decode needs no option: the
 * file's header names the coder.
 * Decode: nx_path as for ntc_decode_file_nx; q_path (NULL: none) = the "NTCQ" file, read once
 * (ntc_q_read); section i belongs to block i of encoded.dat, each batch gets its blocks'
 * sections and the output is FASTQ, "@seq.N\n{read}\n+\n{qualities}\n".  An input that ended
 * cleanly must have used exactly all sections, else NTC_ERR_FORMAT; a damaged encoded.dat
 * keeps ntc_decode_file's semantics (the output ends, dropped_blocks > 0).  The fds and
 * paths of the other direction are ignored.                                                   */
typedef struct ntc_file_opts {
    int32_t nx_policy;   /* NTC_NX_*                                         */
    int32_t nx_fd;       /* encode: exceptions file, -1 = none               */
    int32_t q_mode;      /* 0 drop, 1 keep, 2 bin8                           */
    int32_t q_fd;        /* encode: quality file, -1 = none                  */
    const char *nx_path; /* decode: exceptions file, NULL = none             */
    const char *q_path;  /* decode: quality file, NULL = none                */
} ntc_file_opts;
typedef struct ntc_q_stats {
    uint64_t sections, quals, packed_bytes, deflated_bytes;
} ntc_q_stats;
int ntc_encode_file_ex(ntc_ctx *const *ctxs, int n_ctx, const char *in_path, int out_fd, const ntc_file_opts *fo,
                       const ntc_pipeline_opts *opts, ntc_pipeline_stats *stats, ntc_nx_stats *nx, ntc_q_stats *q);
int ntc_decode_file_ex(ntc_ctx *const *ctxs, int n_ctx, const char *in_path, int out_fd, const ntc_file_opts *fo,
                       const ntc_pipeline_opts *opts, ntc_pipeline_stats *stats);

/* ---- all three side files: exceptions, quality scores and read names ------------------------ */
/* ntc_encode_file_ex2 / ntc_decode_file_ex2 are ntc_encode_file_ex / ntc_decode_file_ex with
 * the name file beside the other two.  ntc_file_opts2 starts with its own size, so that the
 * next side file needs no new entry point: struct_bytes must be at least
 * sizeof(ntc_file_opts2) as declared here, else NTC_ERR_INVALID_ARG.
 * Encode: n_mode 0 (drop): no name file, n_fd must be -1.  n_mode 1 (keep) or 2 (id,
 * ntcomp_codec.h): every block written to encoded.dat gets its name section in the "NTCN"
 * file at n_fd (>= 0, not closed), front-coded on the GPU and deflated by the pipeline's pool
 * with the block's streams; a block the pipeline drops takes its section with it.
 * encoded.dat is byte for byte that of a run without names, and the side file does not depend
 * on the number of contexts or on whether the same text came plain or compressed.  Names
 * exist only where the GPU parses the FASTQ text: host_parse = 1, an input that is not FASTQ,
 * and a batch that falls back to the host parser (a blank line) are NTC_ERR_UNSUPPORTED under
 * modes 1 and 2, with the case in stats->error.  The contexts' "names" option is set for the
 * call and left at 0.  n (may be NULL): sections and names written, their bytes.
 * Decode: n_path (NULL: none) = the "NTCN" file, read once (ntc_n_read); section i belongs to
 * block i of encoded.dat and the output carries the names, ">{name}\n{read}\n" or, with
 * q_path, "@{name}\n{read}\n+\n{qualities}\n".  An input that ended cleanly must have used
 * exactly all sections, else NTC_ERR_FORMAT.  A "+name" third line is not kept: it comes back
 * as a bare "+".                                                                             */
typedef struct ntc_file_opts2 {
    uint32_t struct_bytes; /* sizeof(ntc_file_opts2)                           */
    int32_t nx_policy;     /* NTC_NX_*                                         */
    int32_t nx_fd;         /* encode: exceptions file, -1 = none               */
    int32_t q_mode;        /* 0 drop, 1 keep, 2 bin8                           */
    int32_t q_fd;          /* encode: quality file, -1 = none                  */
    const char *nx_path;   /* decode: exceptions file, NULL = none             */
    const char *q_path;    /* decode: quality file, NULL = none                */
    int32_t n_mode;        /* 0 drop, 1 keep, 2 id                             */
    int32_t n_fd;          /* encode: name file, -1 = none                     */
    const char *n_path;    /* decode: name file, NULL = none                   */
} ntc_file_opts2;
typedef struct ntc_n_stats {
    uint64_t sections, names, name_bytes, payload_bytes, deflated_bytes;
} ntc_n_stats;
int ntc_encode_file_ex2(ntc_ctx *const *ctxs, int n_ctx, const char *in_path, int out_fd, const ntc_file_opts2 *fo,
                        const ntc_pipeline_opts *opts, ntc_pipeline_stats *stats, ntc_nx_stats *nx, ntc_q_stats *q,
                        ntc_n_stats *n);
int ntc_decode_file_ex2(ntc_ctx *const *ctxs, int n_ctx, const char *in_path, int out_fd, const ntc_file_opts2 *fo,
                        const ntc_pipeline_opts *opts, ntc_pipeline_stats *stats);

/* ---- the digest file: a decode that checks itself ------------------------------------------- */
/* ntc_encode_file_ex3 / ntc_decode_file_ex3 are ntc_encode_file_ex2 / ntc_decode_file_ex2 with
 * the per-block content digests of ntcomp_codec.h beside the three side files.  ntc_file_opts3
 * holds ntc_file_opts2's fields in the same order, then its own; struct_bytes must be at least
 * sizeof(ntc_file_opts3) as declared here, else NTC_ERR_INVALID_ARG.
 * Encode: d_mode 0: no digest file, d_fd must be -1.  d_mode 1: every block written to
 * encoded.dat gets its 56-byte section in the "NTCD" file at d_fd (>= 0, not closed), in file
 * order, digested on the GPU from the bytes the call has there anyway; a block the pipeline
 * drops takes its section with it.  The header names the uploaded index (k, n_nodes) and the
 * components the call's modes yield: seq always, sym under NTC_NX_KEEP, qual under q_mode 1 / 2,
 * name under n_mode 1 / 2.  It works with every policy, mode and input kind; encoded.dat and the
 * other side files are byte for byte those of a run without it, and the file does not depend on
 * the number of contexts or on whether the same text came plain or compressed.  The contexts'
 * "digests" option is set for the call and left at 0.  d (may be NULL): sections written, and
 * how many of them hold each component.
 * Decode: d_path (NULL: none) = the "NTCD" file, read once (ntc_d_read).  A file whose k or
 * n_nodes are not the uploaded index's fails before the first batch with NTC_ERR_DIGEST and
 * "written against another index" in stats->error.  Section i belongs to block i of
 * encoded.dat; each batch is checked on the GPU before its text is formatted.  A block that
 * differs ends the call with NTC_ERR_DIGEST: stats->bad_read = the block's first read (from 0,
 * as decode numbers them), stats->error names the block, the component and both values, and the
 * output is a prefix of the true text (the batches before that block's).  Under a digest file
 * the lenient endings of ntc_decode_file are errors: a damaged block or a truncated input is
 * NTC_ERR_FORMAT, not NTC_OK with dropped_blocks > 0, and so are sections left over after a
 * clean end.  A component whose side file is not given (sym: nx_path, qual: q_path, name:
 * n_path) cannot be checked; d->not_checkable collects those bits.  d (may be NULL): sections
 * used, and how many blocks were checked for each component.
 * out_fd = -1 (here only): everything runs, the formatter included, but the text is neither
 * copied off the device nor written -- a verification pass.                                     */
typedef struct ntc_file_opts3 {
    uint32_t struct_bytes; /* sizeof(ntc_file_opts3)                           */
    int32_t nx_policy;     /* NTC_NX_*                                         */
    int32_t nx_fd;         /* encode: exceptions file, -1 = none               */
    int32_t q_mode;        /* 0 drop, 1 keep, 2 bin8                           */
    int32_t q_fd;          /* encode: quality file, -1 = none                  */
    const char *nx_path;   /* decode: exceptions file, NULL = none             */
    const char *q_path;    /* decode: quality file, NULL = none                */
    int32_t n_mode;        /* 0 drop, 1 keep, 2 id                             */
    int32_t n_fd;          /* encode: name file, -1 = none                     */
    const char *n_path;    /* decode: name file, NULL = none                   */
    int32_t d_mode;        /* 0 none, 1 write digests                          */
    int32_t d_fd;          /* encode: digest file, -1 = none                   */
    const char *d_path;    /* decode: digest file, NULL = none                 */
} ntc_file_opts3;
typedef struct ntc_d_stats {
    uint64_t sections;                                      /* written (encode) / checked (decode)  */
    uint64_t blocks_seq, blocks_sym, blocks_qual, blocks_name; /* of them, with / checked for each  */
    uint32_t not_checkable;                                 /* decode: NTC_DIGEST_* present, not checked */
    uint32_t reserved;
} ntc_d_stats;
int ntc_encode_file_ex3(ntc_ctx *const *ctxs, int n_ctx, const char *in_path, int out_fd, const ntc_file_opts3 *fo,
                        const ntc_pipeline_opts *opts, ntc_pipeline_stats *stats, ntc_nx_stats *nx, ntc_q_stats *q,
                        ntc_n_stats *n, ntc_d_stats *d);
int ntc_decode_file_ex3(ntc_ctx *const *ctxs, int n_ctx, const char *in_path, int out_fd, const ntc_file_opts3 *fo,
                        const ntc_pipeline_opts *opts, ntc_pipeline_stats *stats, ntc_d_stats *d);

/* ---- paired-end reads: two mate files in, two out -------------------------------------------- */
/* ntc_encode_file_ex4 / ntc_decode_file_ex4 are ntc_encode_file_ex3 / ntc_decode_file_ex3 for
 * paired archives (ntcomp_codec.h "paired-end reads": read 2p is mate 1 of pair p, read 2p + 1
 * its mate 2; no format changes).  ntc_file_opts4 holds ntc_file_opts3's fields in the same
 * order, then its own; struct_bytes must be at least sizeof(ntc_file_opts4).  pair_mode 0: the
 * calls are the ex3 ones (mate_path must be NULL, out_fd2 -1).  pair_mode 1 (mates checked by
 * their ids) or 2 (not checked):
 * Encode: with mate_path, in_path holds the mate-1 records and mate_path the mate-2 records;
 * both go through the same ingest (mapped plain, or streamed from any supported compression,
 * not necessarily the same), a batch is n records of each -- 2 n a multiple of 65,536, or the
 * inputs' end -- and the GPU weaves them (ntc_encode_pack_fastq_paired).  encoded.dat and the
 * side files are byte for byte those of a single-file encode of the interleaved file, whatever
 * the number of contexts and the compression of either input.  One input ending while the other
 * still holds a record is NTC_ERR_FORMAT, "mate files hold different numbers of records" in
 * stats->error.  Without mate_path, in_path is interleaved: the check is the only new work, and
 * an odd number of reads is NTC_ERR_FORMAT.  A pair whose mates disagree (mode 1) ends the call
 * with NTC_ERR_FORMAT and stats->bad_read = the file index of its mate 1.  Pairs exist only where
 * the GPU parses the text: host_parse = 1, an input that is not FASTQ and a batch that needs the
 * host parser (a blank line, records that are not four lines each) are NTC_ERR_UNSUPPORTED, with
 * the case in stats->error.  The contexts' "paired" option is set for the call and left at 0.
 * p (may be NULL): pairs encoded, the mode, the text bytes of each mate.
 * Decode: out_fd gets the mate-1 records of every batch and out_fd2 (>= 0, not closed) the
 * mate-2 records, in batch order; out_fd2 < 0 is NTC_ERR_INVALID_ARG unless out_fd is -1 (the
 * verification pass, which splits nothing).  The side files work as ever, keyed by the read's
 * index in the archive; without a name file the reads keep the archive's numbering (seq.1,
 * seq.3, ... in out_fd).  p: pairs decoded, the bytes written to each.
 * With the GPU stage's hook table null (a build without it), pair_mode != 0 is
 * NTC_ERR_UNSUPPORTED.                                                                         */
typedef struct ntc_file_opts4 {
    uint32_t struct_bytes; /* sizeof(ntc_file_opts4)                           */
    int32_t nx_policy;     /* NTC_NX_*                                         */
    int32_t nx_fd;         /* encode: exceptions file, -1 = none               */
    int32_t q_mode;        /* 0 drop, 1 keep, 2 bin8                           */
    int32_t q_fd;          /* encode: quality file, -1 = none                  */
    const char *nx_path;   /* decode: exceptions file, NULL = none             */
    const char *q_path;    /* decode: quality file, NULL = none                */
    int32_t n_mode;        /* 0 drop, 1 keep, 2 id                             */
    int32_t n_fd;          /* encode: name file, -1 = none                     */
    const char *n_path;    /* decode: name file, NULL = none                   */
    int32_t d_mode;        /* 0 none, 1 write digests                          */
    int32_t d_fd;          /* encode: digest file, -1 = none                   */
    const char *d_path;    /* decode: digest file, NULL = none                 */
    int32_t pair_mode;     /* 0 off, 1 pairs + mate check, 2 pairs, no check   */
    const char *mate_path; /* encode: the mate-2 input, NULL = in_path is interleaved */
    int32_t out_fd2;       /* decode: the mate-2 text, -1 = none               */
} ntc_file_opts4;
typedef struct ntc_p_stats {
    uint64_t pairs;        /* encoded / decoded                                */
    uint64_t bytes1, bytes2; /* text of each mate read (encode, mate_path) / written (decode) */
    uint32_t mode;         /* the pair_mode of the call                        */
    uint32_t reserved;
} ntc_p_stats;
int ntc_encode_file_ex4(ntc_ctx *const *ctxs, int n_ctx, const char *in_path, int out_fd, const ntc_file_opts4 *fo,
                        const ntc_pipeline_opts *opts, ntc_pipeline_stats *stats, ntc_nx_stats *nx, ntc_q_stats *q,
                        ntc_n_stats *n, ntc_d_stats *d, ntc_p_stats *p);
int ntc_decode_file_ex4(ntc_ctx *const *ctxs, int n_ctx, const char *in_path, int out_fd, const ntc_file_opts4 *fo,
                        const ntc_pipeline_opts *opts, ntc_pipeline_stats *stats, ntc_d_stats *d, ntc_p_stats *p);

/* ---- a range of reads: seek by block, window the text ------------------------------------------ */
/* ntc_archive_info (host only, no context): the blocks of the encoded.dat at path, from their
 * stream headers alone -- nothing is inflated.  *blocks (freed with ntc_buffer_free; null when
 * there are none): byte offset and length, reads (BlockHeader.num_records), records (the flag
 * stream's num_u64) and bad = 1 for a block whose headers cannot describe their gzip streams
 * (its reads and records are then 0: the numbering of every read after it is unknown).
 * *n_reads / *n_records sum the blocks that are not bad; *tail_bytes = the bytes after the last
 * whole block (0 for a file that ends cleanly).  Any output but blocks may be null.
 * NTC_ERR_IO if the file cannot be read.
 *
 * ntc_decode_file_ex5 is ntc_decode_file_ex4 for reads [read_first, read_first + read_count) of
 * the archive, counted from 0.  ntc_file_opts5 holds ntc_file_opts4's fields in the same order,
 * then its own; struct_bytes must be at least sizeof(ntc_file_opts5).  read_count = 0: the whole
 * file, exactly as ntc_decode_file_ex4 decodes it (read_first is ignored).  Otherwise only the
 * blocks that hold the range are inflated and decoded -- the gzip payload of a skipped block is
 * never inflated -- and of the first and last of them only the range's reads are formatted
 * (ntc_decode_set_window); every read keeps its number in the archive (seq.N), its name, its
 * qualities and its exception runs, and the digests of the touched blocks are checked whole.
 * The texts of ranges that partition the archive, concatenated, are the full decode byte for
 * byte.  Under pair_mode both numbers must be even.
 * A range request is strict, as a decode under a digest file is: NTC_ERR_FORMAT, with the case
 * in stats->error, for a bad block anywhere up to the range's last block, a touched block that
 * does not inflate or decodes to another read count than its header's, a side file (quality,
 * name, digest) whose section count differs from the archive's block count or a section whose
 * n_reads differs from its block's header (both checked before any GPU call, from metadata
 * alone).  NTC_ERR_INVALID_ARG, with the archive's read count in stats->error: read_first >=
 * the archive's reads, or read_first + read_count > them.
 * stats: blocks = the touched blocks, reads = the reads written, bases = the bases decoded
 * (those of the touched blocks), bytes_out = the text written.  r (may be NULL): the
 * archive's blocks and reads, the first touched block and how many, the reads written, and the
 * reads of the first / last touched block left out of the text.                                 */
typedef struct ntc_archive_block {
    uint64_t offset, bytes;    /* the block in the file                            */
    uint64_t reads, records;   /* 0 when bad                                       */
    uint32_t bad;              /* 1: damaged headers                               */
    uint32_t reserved;
} ntc_archive_block;
int ntc_archive_info(const char *path, ntc_archive_block **blocks, uint64_t *n_blocks, uint64_t *n_reads,
                     uint64_t *n_records, uint64_t *tail_bytes);

typedef struct ntc_file_opts5 {
    uint32_t struct_bytes; /* sizeof(ntc_file_opts5)                           */
    int32_t nx_policy;     /* NTC_NX_*                                         */
    int32_t nx_fd;         /* encode: exceptions file, -1 = none               */
    int32_t q_mode;        /* 0 drop, 1 keep, 2 bin8                           */
    int32_t q_fd;          /* encode: quality file, -1 = none                  */
    const char *nx_path;   /* decode: exceptions file, NULL = none             */
    const char *q_path;    /* decode: quality file, NULL = none                */
    int32_t n_mode;        /* 0 drop, 1 keep, 2 id                             */
    int32_t n_fd;          /* encode: name file, -1 = none                     */
    const char *n_path;    /* decode: name file, NULL = none                   */
    int32_t d_mode;        /* 0 none, 1 write digests                          */
    int32_t d_fd;          /* encode: digest file, -1 = none                   */
    const char *d_path;    /* decode: digest file, NULL = none                 */
    int32_t pair_mode;     /* 0 off, 1 pairs + mate check, 2 pairs, no check   */
    const char *mate_path; /* encode: the mate-2 input, NULL = in_path is interleaved */
    int32_t out_fd2;       /* decode: the mate-2 text, -1 = none               */
    uint64_t read_first;   /* decode: the range's first read, from 0           */
    uint64_t read_count;   /* decode: its reads, 0 = the whole file            */
} ntc_file_opts5;
typedef struct ntc_r_stats {
    uint64_t blocks_total, reads_total; /* the archive's                                  */
    uint64_t first_block, blocks_read;  /* the touched blocks                             */
    uint64_t reads_written;
    uint64_t head_skipped, tail_skipped; /* reads of the first / last touched block not written */
} ntc_r_stats;
int ntc_decode_file_ex5(ntc_ctx *const *ctxs, int n_ctx, const char *in_path, int out_fd, const ntc_file_opts5 *fo,
                        const ntc_pipeline_opts *opts, ntc_pipeline_stats *stats, ntc_d_stats *d, ntc_p_stats *p,
                        ntc_r_stats *r);

/* ---- BGZF input inflated on the GPU --------------------------------------------------------- */
/* ntc_encode_file_ex6 is ntc_encode_file_ex4 with the engine that inflates a BGZF input.
 * ntc_file_opts6 holds ntc_file_opts5's fields in the same order (the range of reads is not read
 * here), then its own; struct_bytes must be at least sizeof(ntc_file_opts6).
 *   NTC_INFLATE_HOST (0)  as ever: libdeflate on the reader's threads
 *   NTC_INFLATE_GPU  (1)  the reader hands every run of whole BGZF members to an inflater on the
 *                         first context's device (ntc_inflate_members' decoder; DESIGN.md section
 *                         27): compressed bytes up, text down into the reader's buffer at the
 *                         offsets the ISIZE fields give.  Everything after that is unchanged, so
 *                         encoded.dat and every side file are byte for byte those of the host
 *                         engine.  A run in which any member fails is not delivered and goes
 *                         through the host's path, members, errors and exit status as ever; a
 *                         tail that is not BGZF and a member larger than the room left take the
 *                         host's paths too.
 * Under NTC_INFLATE_GPU: NTC_ERR_INVALID_ARG with host_parse = 1; NTC_ERR_UNSUPPORTED, the case in
 * stats->error, when in_path or mate_path does not start with a BGZF member, and when the GPU
 * stage's hook table is null (a build without it).  Any other engine is NTC_ERR_INVALID_ARG.
 * i (may be NULL): the engine, the members and text bytes inflated on the device, the runs
 * handed to it and those that fell back, and the seconds spent inside the inflater.            */
#define NTC_INFLATE_HOST 0
#define NTC_INFLATE_GPU 1
typedef struct ntc_file_opts6 {
    uint32_t struct_bytes; /* sizeof(ntc_file_opts6)                           */
    int32_t nx_policy;     /* NTC_NX_*                                         */
    int32_t nx_fd;         /* encode: exceptions file, -1 = none               */
    int32_t q_mode;        /* 0 drop, 1 keep, 2 bin8                           */
    int32_t q_fd;          /* encode: quality file, -1 = none                  */
    const char *nx_path;   /* decode: exceptions file, NULL = none             */
    const char *q_path;    /* decode: quality file, NULL = none                */
    int32_t n_mode;        /* 0 drop, 1 keep, 2 id                             */
    int32_t n_fd;          /* encode: name file, -1 = none                     */
    const char *n_path;    /* decode: name file, NULL = none                   */
    int32_t d_mode;        /* 0 none, 1 write digests                          */
    int32_t d_fd;          /* encode: digest file, -1 = none                   */
    const char *d_path;    /* decode: digest file, NULL = none                 */
    int32_t pair_mode;     /* 0 off, 1 pairs + mate check, 2 pairs, no check   */
    const char *mate_path; /* encode: the mate-2 input, NULL = in_path is interleaved */
    int32_t out_fd2;       /* decode: the mate-2 text, -1 = none               */
    uint64_t read_first;   /* decode: the range's first read, from 0           */
    uint64_t read_count;   /* decode: its reads, 0 = the whole file            */
    int32_t inflate_engine; /* encode: NTC_INFLATE_*                           */
    int32_t reserved;      /* 0                                                */
} ntc_file_opts6;
typedef struct ntc_i_stats {
    uint32_t engine;       /* the inflate_engine of the call                   */
    uint32_t reserved;
    uint64_t members;      /* BGZF members inflated on the device              */
    uint64_t bytes;        /* their text                                       */
    uint64_t runs;         /* runs of members handed to the inflater           */
    uint64_t fallback_runs; /* ... that were not delivered: a member failed    */
    double seconds;        /* inside the inflater: copies, kernel, waiting     */
} ntc_i_stats;
int ntc_encode_file_ex6(ntc_ctx *const *ctxs, int n_ctx, const char *in_path, int out_fd, const ntc_file_opts6 *fo,
                        const ntc_pipeline_opts *opts, ntc_pipeline_stats *stats, ntc_nx_stats *nx, ntc_q_stats *q,
                        ntc_n_stats *n, ntc_d_stats *d, ntc_p_stats *p, ntc_i_stats *i);

/* ---- decoded text written as BGZF, compressed on the GPU ------------------------------------ */
/* ntc_decode_file_ex7 is ntc_decode_file_ex5 with the output's format.  ntc_file_opts7 holds
 * ntc_file_opts6's fields in the same order (inflate_engine is not read here), then its own;
 * struct_bytes must be at least sizeof(ntc_file_opts7).
 *   NTC_OUT_TEXT (0)  as ever: the text.
 *   NTC_OUT_BGZF (1)  every batch's text is cut into BGZF members at record boundaries and
 *                     compressed on the device that formatted it (the context option "bgzf_text",
 *                     ntc_bgzf_compress's plan and coder); only the members
 *                     cross to the host.  They are written in batch order, and the 28-byte EOF
 *                     member (NTC_BGZF_EOF) is appended only when the call returns NTC_OK: a
 *                     decode that fails -- a digest mismatch, a damaged block under a range --
 *                     leaves a file without the marker, which is how BGZF tools tell a truncated
 *                     file.  Under pairs out_fd and out_fd2 are each a BGZF file of their own.
 *                     Members never span a batch, so for a given blocks_per_batch the bytes do
 *                     not depend on the contexts or threads; across batch sizes only the inflated
 *                     text is the same.  The outputs of ranges that partition the archive,
 *                     concatenated, are a BGZF file of the whole text (an EOF member in the middle
 *                     is an empty member).  out_fd -1 wins: nothing is compressed.
 * NTC_ERR_UNSUPPORTED for NTC_OUT_BGZF when the GPU stage's hook table is null (a build without
 * it); any other format, or a non-zero reserved2, is NTC_ERR_INVALID_ARG.
 * z (may be NULL): the format, the members written (the EOF members not counted), their text and
 * bytes, the chunks by the encoding chosen, and the seconds the contexts spent making them.      */
#define NTC_OUT_TEXT 0
#define NTC_OUT_BGZF 1
typedef struct ntc_file_opts7 {
    uint32_t struct_bytes; /* sizeof(ntc_file_opts7)                           */
    int32_t nx_policy;     /* NTC_NX_*                                         */
    int32_t nx_fd;         /* encode: exceptions file, -1 = none               */
    int32_t q_mode;        /* 0 drop, 1 keep, 2 bin8                           */
    int32_t q_fd;          /* encode: quality file, -1 = none                  */
    const char *nx_path;   /* decode: exceptions file, NULL = none             */
    const char *q_path;    /* decode: quality file, NULL = none                */
    int32_t n_mode;        /* 0 drop, 1 keep, 2 id                             */
    int32_t n_fd;          /* encode: name file, -1 = none                     */
    const char *n_path;    /* decode: name file, NULL = none                   */
    int32_t d_mode;        /* encode: 0 off, 1 digests                         */
    int32_t d_fd;          /* encode: digest file, -1 = none                   */
    const char *d_path;    /* decode: digest file, NULL = none                 */
    int32_t pair_mode;     /* 0 off, 1 pairs + mate check, 2 pairs, no check   */
    const char *mate_path; /* encode: the mate-2 input, NULL = in_path is interleaved */
    int32_t out_fd2;       /* decode: the mate-2 text, -1 = none               */
    uint64_t read_first;   /* decode: the range's first read, from 0           */
    uint64_t read_count;   /* decode: its reads, 0 = the whole file            */
    int32_t inflate_engine; /* encode: NTC_INFLATE_*                           */
    int32_t reserved;      /* 0                                                */
    int32_t out_format;    /* decode: NTC_OUT_*                                */
    int32_t reserved2;     /* 0                                                */
} ntc_file_opts7;
typedef struct ntc_z_stats {
    uint32_t out_format;   /* the out_format of the call                       */
    uint32_t reserved;
    uint64_t members;      /* BGZF members written, the EOF members not counted */
    uint64_t text_bytes;   /* the text they hold                               */
    uint64_t bytes;        /* their bytes                                      */
    uint64_t chunks_stored, chunks_huffman, chunks_matches; /* by the encoding chosen */
    double seconds;        /* the contexts' time in the plan, the coder and the members' copy */
} ntc_z_stats;
int ntc_decode_file_ex7(ntc_ctx *const *ctxs, int n_ctx, const char *in_path, int out_fd, const ntc_file_opts7 *fo,
                        const ntc_pipeline_opts *opts, ntc_pipeline_stats *stats, ntc_d_stats *d, ntc_p_stats *p,
                        ntc_r_stats *r, ntc_z_stats *z);

#ifdef __cplusplus
}
#endif
#endif
