// Kernel argument structs and launchers (kernels.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "encode_core.h"

namespace ntc {

struct HostIndex;
// GPU index build (build.hip): the host builder's index (sbwt_build.cpp), built on stream s
// in bucket-range partitions whose passes fit device_budget (0: 85 % of the free HBM);
// sorted partitions wait in host memory up to host_budget (0: no limit), past it in files
// under temp_dir.  max_partition_keys caps a pass (test hook, 0: from the budget).
struct BuildOpts {
    uint64_t device_budget = 0, host_budget = 0, max_partition_keys = 0;
    std::string temp_dir;
};
struct BuildStats {
    uint64_t occurrences = 0, kmers = 0, sources = 0, nodes = 0;
    uint64_t spilled_bytes = 0, device_budget = 0, pass_keys = 0, peak_device_bytes = 0;
    uint32_t kmer_partitions = 0, node_partitions = 0, compactions = 0, seq_uploads = 0;
    double seconds = 0, seconds_kmers = 0, seconds_sources = 0, seconds_nodes = 0, seconds_labels = 0;
    double seconds_plan = 0, seconds_sort = 0;  // the occurrence histogram (sequence upload included); sorts
};
bool build_index_device(hipStream_t s, const uint8_t *seqs, const uint64_t *offs, uint64_t n_seqs, uint32_t k,
                        bool revcomp, const BuildOpts &o, HostIndex &out, BuildStats &st, std::string &err);

struct EncodeArgs {
    DevIndex ix;
    const uint8_t *bases;
    const uint64_t *offs;        // [n_reads+1], absolute into bases
    uint64_t n_reads;
    const uint64_t *tile_base;   // [tiles+1] scratch rows per tile, or null => uniform
    uint64_t rows_uniform;       // multiple of 32
    uint8_t *D;
    uint32_t *S;
    uint32_t *F;
    uint64_t *R;
    uint32_t *rec_count;
    unsigned long long *status;  // min over (read << 8 | code); ~0 = ok
};

struct Enc4Args {
    DevIndex ix;
    const uint8_t *bases;
    const uint64_t *offs;        // [n_reads+1], absolute into bases
    uint64_t n_reads;
    uint64_t *Q;                 // packed bases, position space (2 bits, 32 per word)
    Entry *Es;                   // the next S entries of each read (secondary slots, ent_ptr)
    uint32_t S;                  // secondary slots per read (multiple of 4)
    Entry *Ep;                   // overflow pool of entries (reservations, MsLaneT::reserve)
    uint64_t pcap;               // its entries (< 2^32)
    uint32_t *obase;             // each overflowing read's entry reservation
    Entry *Ed;                   // first kEntSlot entries of each read (dense slots, ent_ptr)
    uint32_t *ne;                // entries per read
    uint64_t *R;                 // records past kRecSlot: reservations (parse_read's RecPool)
    uint64_t rcap;               // its records (< 2^32)
    uint32_t *rbase;             // each overflowing read's record reservation
    uint64_t *R2;                // first kRecSlot records of each read (dense slots)
    uint32_t *rec_count;
    uint32_t *wave_cnt;          // records of each wave's 64 reads (k_parse4 -> scan -> k_emit4)
    unsigned long long *status;
    unsigned long long *counter; // work queue heads of k_ms4 (WaveQueue, zeroed per call), then
                                 // the entry and record pool counters (kPoolCounters)
};
// the pools' reservation counters: words 64 and 72 of the counter area (past the 8 queue
// heads, 64 B apart), zeroed with them per call
constexpr uint32_t kPoolCntE = 64, kPoolCntR = 72;

struct EmitArgs {
    const uint64_t *R;           // [tile][j][lane]
    const uint64_t *tile_base;
    uint64_t rows_uniform;
    const uint32_t *rec_count;
    const uint64_t *rec_offsets;
    uint64_t n_reads;
    uint64_t *out;
    uint64_t capacity;
    unsigned long long *status;
};

struct DebugArgs {
    const uint8_t *D;
    const uint32_t *S;
    const uint64_t *tile_base;
    uint64_t rows_uniform;
    const uint64_t *offs;
    uint64_t n_reads;
    uint32_t *d_out;
    uint32_t *s_out;
};

// decode tiles: k_dec_rec's block of 256 threads owns kDecTileRecs consecutive records, kDecR
// per thread (independent walk chains per lane).  4: 126 VGPRs, 4 waves/SIMD = 16 chains per
// SIMD (2: 84 VGPRs, 5 waves = 10 chains); D91 k_dec_rec 0.935 -> 0.900 ms, SD91 1.117 ->
// 1.103 ms (A/B on one box, round 3)
#ifndef NTC_DEC_R
#define NTC_DEC_R 4
#endif
constexpr uint32_t kDecR = NTC_DEC_R;
constexpr uint32_t kDecTileRecs = 256 * kDecR;

struct DecWalkArgs {
    DevIndex ix;
    const uint64_t *recs;
    uint64_t n;
    const uint64_t *pfs;         // per kDecTileRecs-record tile: first records before it [tiles + 1]
    const uint64_t *pls;         // per tile: bases before it [tiles + 1]
    uint64_t *offs_out;          // each read's output offset [nreads + 1] (written here)
    uint64_t offs_capacity;
    uint64_t bases_capacity;
    uint8_t *out;
    unsigned long long *status;
};

// GPU block packer (pack.hip): per 65,536-read block, stream totals, then the four coded
// streams of write_block_to (src/lib.rs:232-252) before deflate
struct PackStats {
    uint64_t n_recs, n_long, max1, sum2, sum3, T, max4, bad, rec_begin;
};
struct PackParams {
    uint64_t off[4];      // word offsets of s1..s4 in the payload
    uint64_t lim1, lim4;  // minimal-binary limits 2^(l+1) - max
    int32_t p2, p3, l1, l4;
    uint32_t skip, pad;   // skip: the block is dropped (App. B.3) or malformed
    uint32_t seg0, nseg;  // the block's pass-2 segments [seg0, seg0 + nseg): records first, then s4 chunks
};
// a workgroup's share of pass 2: kind 0 = records [first, first + count) (absolute indices,
// streams s1-s3), kind 1 = s4 chunks [first, first + count) of the block
struct PackSeg {
    uint32_t block, kind;
    uint64_t first, count;
};
constexpr uint64_t kPackSegRecs = 16384, kPackSegChunks = 16384;
// pass 1 (stream totals + s4 chunks) in segments of 4096 reads: chunks (chunk_words words,
// zeroed here) as pack.hip chunk_base lays them out, scratch: pack_stats_scratch_words()
uint64_t pack_stats_scratch_words(uint64_t n_blocks, uint32_t block_reads);
void launch_pack_stats(const uint64_t *recs, const uint64_t *roffs, uint64_t n_reads, uint32_t block_reads,
                       uint64_t n_blocks, uint64_t *chunks, uint64_t chunk_words, uint64_t *scratch,
                       PackStats *stats, hipStream_t s);
// pass 2 over n_segs segments: their code lengths, each block's segment offsets (seg_bits /
// seg_start: 3 words per segment), then every segment's codes in parallel
void launch_pack_write(const uint64_t *recs, const uint64_t *chunks, const PackStats *stats,
                       const PackParams *params, uint64_t n_blocks, const PackSeg *segs, uint64_t n_segs,
                       uint64_t *seg_bits, uint64_t *seg_start, uint64_t *payload, uint64_t *bits_out,
                       hipStream_t s);

// decode output as FASTA text on the GPU (fasta.hip): ">seq.{first_id + r}\n{read r}\n";
// sizes / out_offs: n + 1 words, tmp: scan_tmp_words(n) words; out_offs[n] = total bytes.
// Nothing is written unless the decode status is clear (~0) and the text fits out_cap.
// GPU block unpacker (unpack.hip): stream i of block b is entry 4 b + i (s1 colex, s2 length,
// s3 flag, s4 short-base chunks), its inflated big-endian words at payload[word_off ...]
struct UnpackStream {
    uint64_t word_off;  // u64 words into the payload (and into the marks scratch)
    uint64_t nwords;    // encoded_size
    uint64_t n;         // num_u64 values
    uint64_t param;     // Rice parameter / minimal-binary max
    uint64_t val_off;   // its values at vals[val_off ...]
};
// The streams run in tiles (a workgroup each): tile k of a list is tile `tile` of stream si,
// which is entry `stream` of the list's streams; a stream's tiles are contiguous, from
// first_tile.  unpack_plan lists the minimal-binary (s1, s4) and Rice (s2, s3) tiles from the
// host copy of the stream table.
struct UnpTile {
    uint32_t si, tile, stream, pad;
};
struct UnpStreamRef {
    uint32_t si, first_tile, n_tiles, pad;
};
struct UnpackPlan {
    std::vector<UnpTile> mb_tiles, rice_tiles;
    std::vector<UnpStreamRef> mb_streams, rice_streams;
};
void unpack_plan(const UnpackStream *st, uint64_t n_blocks, UnpackPlan &plan);
uint64_t unpack_ws_bytes(const UnpackPlan &plan);  // the tiles' tables (ws)
// streams -> values (status[4 b + i]), zip -> records of block b at recs[rec_off[b] ...];
// out3[3 b .. 3 b + 2] = reads, bases, status, and after the blocks' three words about the
// Rice paths taken (streams flagged not-simple, serial; segments run through).  marks: as
// many words as the payload; segc: unpack_seg_words(n_blocks, the largest block's records) words
struct UnpackDev {
    const uint64_t *payload;
    const UnpackStream *st;
    uint64_t n_blocks, max_recs;
    uint64_t *marks;
    const UnpTile *mb_tiles, *rice_tiles;  // the plan's lists, on the device
    const UnpStreamRef *mb_streams, *rice_streams;
    uint32_t n_mb_tiles, n_rice_tiles, n_mb_streams, n_rice_streams;
    void *ws;
    uint64_t *vals;
    int32_t *status;
    const uint64_t *rec_off;
    uint64_t *recs, *segc, *out3;
};
void launch_unpack(const UnpackDev &d, hipStream_t s);
uint64_t unpack_seg_words(uint64_t n_blocks, uint64_t max_recs);
void launch_fasta(const uint8_t *d_bases, const uint64_t *d_offs, uint64_t n, uint64_t first_id,
                  const unsigned long long *d_status, uint64_t *sizes, uint64_t *out_offs, uint64_t *tmp, uint8_t *out,
                  uint64_t out_cap, hipStream_t s, uint64_t w_first = 0, uint64_t w_count = 0);
// A window on the formatters (window.hip, window_core.h): w_count != 0 in launch_fasta,
// launch_fastq_text and launch_named_text formats only reads [w_first, w_first + w_count) of
// the n (a valid window, w_valid), packed at the head of out; out_offs[n] = their bytes.
// launch_window_sizes zeroes the sizes outside the window (the formatters call it before their
// scan); launch_window_box: box[13] = *total.  Without a window neither is launched.
void launch_window_sizes(uint64_t *sizes, uint64_t n, uint64_t first, uint64_t count, hipStream_t s);
void launch_window_box(const uint64_t *total, uint64_t *box, hipStream_t s);

// plain FASTQ text of n_reads whole 4-line records -> normalised bases + read offsets
// (fastq.hip).  tile_cnt: fastq_tiles(n_raw) words, tile_base: tiles + 1 (its last word =
// the newlines found), nl: 4 n_reads, kept: n_reads, offs: n_reads + 1, tmp:
// scan_tmp_words(max(tiles, n_reads) + 1), bases: room for the sequence lines' bytes.
// status (preset to ~0) gets read << 8 | NTC_ERR_FORMAT for the first malformed record;
// then no base is written.
struct FastqArgs {
    const uint8_t *raw;
    uint64_t n_raw, n_reads;
    uint32_t *tile_cnt;
    uint64_t *tile_base;
    uint32_t *nl;
    uint32_t *kept;
    uint64_t *offs;
    uint64_t *tmp;
    uint8_t *bases;
    unsigned long long *status;
};
uint64_t fastq_tiles(uint64_t n_raw);
void launch_fastq_parse(const FastqArgs &a, hipStream_t s);
// its first two passes alone: the positions of the first nl_cap newlines of raw, in order, and
// tile_base[fastq_tiles(n_raw)] = the newlines found (tile_cnt, tile_base, tmp as above)
void launch_fastq_lines(const uint8_t *raw, uint64_t n_raw, uint32_t *tile_cnt, uint64_t *tile_base, uint32_t *nl,
                        uint64_t nl_cap, uint64_t *tmp, hipStream_t s);

// Paired-end reads (pairs.hip, pair_core.h).  The weave: two FASTQ texts of n_pairs records
// each (raw[t] 16-byte aligned, nl[t] / n_nl_p[t] from launch_fastq_lines with nl_cap = 4
// n_pairs) -> out, record p of text 1 then record p of text 2, a newline added after a last
// line that lacks one; out_bytes = the woven size (the host knows it: both texts and the
// newlines added).  sizes: n_pairs + 1 words, offs: n_pairs + 1, tmp: scan_tmp_words(n_pairs).
// status: the weave's own word (preset here), read << 8 | NTC_ERR_FORMAT when a text does not
// hold exactly 4 n_pairs lines; then nothing is woven.
struct PairWeaveArgs {
    const uint8_t *raw[2];
    uint64_t n_raw[2];
    const uint32_t *nl[2];
    const uint64_t *n_nl_p[2];
    uint64_t n_pairs;
    uint32_t *sizes;
    uint64_t *offs;
    uint64_t *tmp;
    uint8_t *out;
    uint64_t out_bytes;
    unsigned long long *status;
};
void launch_pair_weave(const PairWeaveArgs &a, hipStream_t s);
// The mate check, after launch_fastq_parse over the interleaved text (its raw, nl and status):
// status, a word of the check's own (preset here), gets (2 p) << 8 | NTC_ERR_FORMAT for the
// lowest pair p whose names disagree.  Nothing is looked at when the parse failed.
struct PairCheckArgs {
    const uint8_t *raw;
    const uint32_t *nl;
    uint64_t n_pairs;
    const unsigned long long *parse_status;
    unsigned long long *status;
};
void launch_pair_check(const PairCheckArgs &a, hipStream_t s);
// box[10] = the weave's status, box[11] = the check's
void launch_pair_box(const unsigned long long *weave, const unsigned long long *check, uint64_t *box, hipStream_t s);
// The split, after a formatter (launch_fasta, launch_fastq_text, launch_named_text) left text
// and out_offs[2 n_pairs + 1]: all even reads' records in order, then all odd reads', into out
// (cap bytes); box[12] = the bytes of the first part.  s1, s2, o1, o2: n_pairs + 1 words each,
// tmp: scan_tmp_words(n_pairs).  Writes nothing when the formatter wrote nothing.
struct PairSplitArgs {
    const uint8_t *text;
    const uint64_t *out_offs;
    uint64_t n_pairs, cap;
    uint64_t *s1, *s2, *o1, *o2, *tmp;
    uint8_t *out;
    uint64_t *box;
};
void launch_pair_split(const PairSplitArgs &a, hipStream_t s);

// Non-ACGT symbols (nonacgt.hip, nonacgt_core.h).  Encode side, over staged (writable)
// bases: M / S / E bitmaps of nx_words(total) words each, cnt_s / cnt_e as many u32, soff /
// eoff one word more (exclusive scans, scan_tmp: scan_tmp_words(words)), counts[0] = runs
// found, counts[1] = bases flagged.  The first run_cap runs go to runs (null: none are
// listed, policy mask); then every flagged byte becomes sub.
struct NxRun;
struct NxArgs {
    uint8_t *bases;
    const uint64_t *offs;   // [n_reads + 1], absolute into bases
    uint64_t n_reads, total, n_words;
    uint64_t *M, *S, *E;
    uint32_t *cnt_s, *cnt_e;
    uint64_t *soff, *eoff;
    uint64_t *counts;
    uint64_t *box;          // the context's host mailbox: words 4, 5 = counts (k_status_box fills 0..3)
    NxRun *runs;
    uint64_t run_cap;
    uint32_t sub;
    unsigned long long *status;
};
uint64_t nx_words(uint64_t total);
void launch_nx_mask(const NxArgs &a, uint64_t *scan_tmp, hipStream_t s);
// Decode side: n pieces (runs, long ones cut into slices) over the decoded bases and read
// offsets; a piece that does not fit, or covers a byte other than sub, sets status to
// read << 8 | NTC_ERR_FORMAT and writes nothing.
struct NxPatchArgs {
    const NxRun *runs;
    uint64_t n;
    uint8_t *bases;
    const uint64_t *offs;   // [n_reads + 1]
    uint64_t n_reads;
    uint32_t sub;
    unsigned long long *status;
};
void launch_nx_patch(const NxPatchArgs &a, hipStream_t s);

// Quality scores (quality.hip, quality_core.h).  Encode side, after launch_fastq_parse over
// the same text: quals = the quality bytes at the reads' base offsets (room for the bases +
// 64), pres: 4 words per block, blocks: n_blocks + 1 entries (the last holds the totals),
// payload: q_payload_words_max(total bases, n_blocks) words.  status: a word of the
// quality pass's own (preset here), read << 8 | NTC_ERR_FORMAT for the first bad read;
// box[6] = that status, box[7] = payload words (the context's host mailbox).
struct QBlock {
    uint64_t n_quals, q_off, word_off, n_words, span_off;
    uint64_t p0, p1;  // presence map, bits 0..127
    uint32_t n_syms, w;
    uint8_t alphabet[96];
    uint64_t body_bytes;  // coder 1 (qrans.hip): the section body's bytes, at byte 8 word_off of the payload
};
struct QEncArgs {
    const uint8_t *raw;
    uint64_t n_raw;
    const uint32_t *nl;
    const uint64_t *n_nl_p;
    const uint64_t *offs;  // [n_reads + 1]
    uint64_t n_reads, n_blocks;
    uint32_t block_reads, mode;
    uint8_t *quals;
    uint32_t *pres;
    QBlock *blocks;
    uint64_t *payload;
    unsigned long long *status;
    uint64_t *box;
};
uint64_t q_payload_words_max(uint64_t total, uint64_t n_blocks);
void launch_quality_pack(const QEncArgs &a, uint64_t total, hipStream_t s);
// the first two steps alone (k_q_gather, k_q_alpha): what both coders start from
void launch_quality_gather(const QEncArgs &a, hipStream_t s);
// Smoothing inside long matches (option "quality_smooth", qsmooth_core.h): the steps one by
// one, since k_q_smooth needs the encode's final records between the first and the rest.
//   launch_quality_lines   k_q_gather alone (presets the status and the presence maps)
//   launch_quality_smooth  the rule in place over quals, the presence maps rebuilt from the
//                          smoothed bytes, *count = bytes replaced (zeroed here)
//   launch_quality_alpha   k_q_alpha alone
//   launch_quality_spans   k_q_pack alone (coder 1: launch_quality_rans instead)
// recs / roffs: the records of the batch and the n_reads + 1 record offsets, from 0.
struct QSmoothArgs {
    QEncArgs q;
    const uint64_t *recs, *roffs;
    uint32_t m, to;  // the options: a trusted record has >= m bases, the target is the mode's image of `to`
    unsigned long long *count;
};
void launch_quality_lines(const QEncArgs &a, hipStream_t s);
void launch_quality_smooth(const QSmoothArgs &a, hipStream_t s);
void launch_quality_alpha(const QEncArgs &a, hipStream_t s);
void launch_quality_spans(const QEncArgs &a, uint64_t total, hipStream_t s);
// Coder 1, the order-1 rANS coder (qrans.hip, qrans_core.h), in place of k_q_pack after
// launch_quality_gather.  With S = qr_spans_max(total, n_blocks): counts: n_blocks *
// kQRCountStride words (zeroed here), cum: n_blocks * kQRCumStride u16, scratch: S *
// kQRSlot + 64 bytes, sizes / offs: S + 1 words each, tmp: scan_tmp_words(S) words, payload
// (q.payload): qr_payload_bytes_max(total, n_blocks) bytes.  Every body starts 8-aligned, the
// bytes up to the next body are zero; box[7] = the payload's 64-bit words, blocks[b].word_off
// and body_bytes say where each body lies.
constexpr uint64_t kQRCountStride = 95 * 94, kQRCumStride = 95 * 96, kQRSlot = 3080;
struct QREncArgs {
    QEncArgs q;
    uint32_t *counts;
    uint16_t *cum;
    uint8_t *scratch;
    uint64_t *sizes, *offs, *tmp;
    uint64_t spans_max;
};
uint64_t qr_spans_max(uint64_t total, uint64_t n_blocks);
uint64_t qr_payload_bytes_max(uint64_t total, uint64_t n_blocks);
void launch_quality_rans(const QREncArgs &a, hipStream_t s);
// Decode side: block b covers reads [r0, r1) of the decoded batch; its codes become bytes
// at those reads' offsets in quals.  A code >= n_syms, or a block whose n_quals is not the
// bases of its reads, sets status (the decode call's) to r0 << 8 | NTC_ERR_FORMAT.
struct QDecBlock {
    uint64_t r0, r1, n_quals, word_off;
    uint32_t w, n_syms;
    uint8_t alphabet[96];
};
struct QDecArgs {
    const QDecBlock *blocks;
    uint64_t n_blocks, tiles;  // tiles: quality_unpack_tiles(the largest n_quals)
    const uint64_t *payload;
    const uint64_t *offs;      // [n_reads + 1]
    uint64_t n_reads;
    uint8_t *quals;
    unsigned long long *status;
};
uint64_t quality_unpack_tiles(uint64_t max_quals);
void launch_quality_unpack(const QDecArgs &a, hipStream_t s);
// Coder 1: block b's body (validated by the host, qr_body_ok) lies at byte body_off (8-aligned)
// of payload, its spans are span_off .. of span_at, which holds two words per span: where its
// stream starts and ends in payload.  Status as above, also for a slot in no symbol, a byte
// needed past the span's end, a final state other than L and unconsumed bytes.
struct QRDecBlock {
    uint64_t r0, r1, n_quals, body_off, span_off;
    uint32_t n_syms, pad;
    uint8_t alphabet[96];
};
struct QRDecArgs {
    const QRDecBlock *blocks;  // [n_blocks + 1]: the last one's span_off = n_spans
    uint64_t n_blocks, n_spans;
    const uint8_t *payload;
    const uint64_t *span_at;
    const uint64_t *offs;      // [n_reads + 1]
    uint64_t n_reads;
    uint8_t *quals;
    unsigned long long *status;
};
void launch_quality_rans_decode(const QRDecArgs &a, hipStream_t s);
// Deflate of the packed streams (deflate.hip, deflate_core.h).  Stream s is chunks first_chunk ..
// + n_chunks, chunk c the n bytes at payload + src_off (last: its stream's last chunk).  With N
// chunks and S streams: tokens: N * kDfChunk words, stage: N * kDfSlot bytes, results: N,
// chunk_off: N words, crcs: S words, member_off_len: 2 S + 1 words (device; pairs of where a
// member starts in out and its bytes, then the total), out: the sum of df_member_bound(n) bytes.
struct DfResult;
struct DfChunkDesc {
    uint64_t src_off;
    uint32_t n, last;
};
struct DfStreamDesc {
    uint64_t n;
    uint32_t first_chunk, n_chunks;
};
struct DfArgs {
    const uint8_t *payload;
    const DfChunkDesc *chunks;
    const DfStreamDesc *streams;
    uint32_t n_chunks, n_streams;
    uint32_t *tokens;
    uint8_t *stage;
    DfResult *results;
    uint64_t *chunk_off;
    uint32_t *crcs;
    uint64_t *member_off_len;
    uint8_t *out;
};
void launch_deflate(const DfArgs &a, hipStream_t s);
// k_df_place alone: chunk c's results[c].size bytes from its slot of stage to out + chunk_off[c]
// (the other fields are not read)
void launch_deflate_place(const DfArgs &a, hipStream_t s);
// BGZF members of a text in HBM (bgzf.hip, bgzf_core.h).  text: n bytes; off (null: plain cuts):
// n_rec + 1 record offsets, off[r] - off_base being record r's start.  With C = bgzf_cells(n, off
// != null), M = bgzf_members_max(n) and N = kBgzfMemberChunks M: cuts / cell_first: C + 1 words
// each, members: M, member_chunk / crcs: M words, chunks / results: N, chunk_off: N words,
// stage: N * kDfSlot bytes, tokens: workgroups * kDfChunk words, counts: 8 words (members,
// chunks, text bytes, output bytes, chunks stored / Huffman / Huffman with matches), out:
// bgzf_bound(n) bytes.  launch_bgzf_plan fills the descriptors and counts[0..2]; the caller reads
// them, sets n_members and n_chunks, and launch_bgzf_code does the rest.
struct BgzfMember;
struct BgzfArgs {
    const uint8_t *text;
    uint64_t n;
    const uint64_t *off;
    uint64_t n_rec, off_base, n_cells;
    uint64_t *cuts, *cell_first;
    BgzfMember *members;
    uint32_t *member_chunk, *crcs;
    DfChunkDesc *chunks;
    DfResult *results;
    uint64_t *chunk_off;
    uint8_t *stage;
    uint32_t *tokens;
    uint64_t *counts;
    uint8_t *out;
    uint64_t max_members, max_chunks;  // the tables' entries: the plan writes no descriptor when it counts more
    uint32_t n_members, n_chunks, workgroups;
};
void launch_bgzf_plan(const BgzfArgs &a, hipStream_t s);
void launch_bgzf_code(const BgzfArgs &a, hipStream_t s);
// Inflate of gzip members (inflate.hip, inflate_core.h).  Member i is the src_bytes bytes at comp +
// src_off and inflates to out_bytes bytes at dst + dst_off (ntc_inflate_member's layout); its
// status, bytes and CRC-32 go to results[i].  Everything is device memory; the caller has checked
// that the members lie inside comp and dst and that no two dst ranges overlap.
struct InfResult;
struct InfMemberDesc {
    uint64_t src_off;
    uint32_t src_bytes, out_bytes;
    uint64_t dst_off;
};
struct InfArgs {
    const uint8_t *comp;
    const InfMemberDesc *members;
    uint32_t n_members;
    uint8_t *dst;
    InfResult *results;
};
void launch_inflate(const InfArgs &a, hipStream_t s);
// launch_fasta's FASTQ twin: "@seq.{first_id + r}\n{read r}\n+\n{qualities r}\n"
void launch_fastq_text(const uint8_t *d_bases, const uint8_t *d_quals, const uint64_t *d_offs, uint64_t n,
                       uint64_t first_id, const unsigned long long *d_status, uint64_t *sizes, uint64_t *out_offs,
                       uint64_t *tmp, uint8_t *out, uint64_t out_cap, hipStream_t s, uint64_t w_first = 0,
                       uint64_t w_count = 0);

// Read names (names.hip, names_core.h).  Encode side, after launch_fastq_parse over the same
// text: start / len / mid: n_reads + 1 words each, ps: two columns of n_reads bytes (pre,
// suf), len_off / mid_off: n_reads + 1 words (exclusive scans, tmp: scan_tmp_words(n_reads)),
// blocks: n_blocks + 1 entries (the last holds the totals), payload: names_payload_max bytes.
// status: a word of the names pass's own (preset here), read << 8 | NTC_ERR_FORMAT for the
// first name past NTC_NAME_MAX; box[8] = that status, box[9] = payload bytes.
struct NBlock {
    uint64_t n_reads, name_bytes, mid_bytes, payload_off, payload_bytes;
};
struct NEncArgs {
    const uint8_t *raw;
    uint64_t n_raw;
    const uint32_t *nl;
    const uint64_t *n_nl_p;
    uint64_t n_reads, n_blocks;
    uint32_t block_reads, mode;
    uint32_t *start, *len, *mid;
    uint8_t *ps;
    uint64_t *len_off, *mid_off, *tmp;
    NBlock *blocks;
    uint8_t *payload;
    unsigned long long *status;
    uint64_t *box;
};
uint64_t names_payload_max(uint64_t n_raw, uint64_t n_reads, uint64_t n_blocks);
void launch_names_pack(const NEncArgs &a, hipStream_t s);
// Decode side: section b covers reads [r0, r1) of the decoded batch and lies at payload +
// payload_off (the host checked its size and place).  len / mid: n_reads + 1 words,
// name_off / mid_off: their exclusive scans, names: names_cap bytes for the expanded names,
// read by read.  Any per-read condition that fails, a section whose mids or names do not
// sum to its meta, sets status (the decode call's) to r << 8 | NTC_ERR_FORMAT.
struct NDecBlock {
    uint64_t r0, r1, name_bytes, mid_bytes, payload_off;
};
struct NDecArgs {
    const NDecBlock *blocks;
    uint64_t n_blocks, max_reads;  // max_reads: the reads of the largest section
    const uint8_t *payload;
    uint64_t payload_bytes;
    uint64_t n_reads;
    uint32_t *len, *mid;
    uint64_t *name_off, *mid_off, *tmp;
    uint8_t *names;
    uint64_t names_cap;
    unsigned long long *status;
};
void launch_names_expand(const NDecArgs &a, hipStream_t s);
// launch_fasta / launch_fastq_text with names: ">{name r}\n{read r}\n", or with d_quals
// "@{name r}\n{read r}\n+\n{qualities r}\n"
void launch_named_text(const uint8_t *d_bases, const uint8_t *d_quals, const uint64_t *d_offs, const uint8_t *d_names,
                       const uint64_t *d_name_off, uint64_t n, const unsigned long long *d_status, uint64_t *sizes,
                       uint64_t *out_offs, uint64_t *tmp, uint8_t *out, uint64_t out_cap, hipStream_t s,
                       uint64_t w_first = 0, uint64_t w_count = 0);

// Per-block content digests (digest.hip, digest_core.h).  A table entry is the public
// ntc_digest_meta: d[c] is the digest of component c (seq, sym, qual, name).
struct DigestMetaDev {
    uint64_t n_reads, n_bases, d[4];
    uint32_t components, pad;
};
// encode: entry b = reads [b block_reads, ...) of offs (n_reads + 1 words), the digests zeroed
// except those whose bit is set in keep
void launch_digest_init(DigestMetaDev *table, uint64_t n_blocks, uint64_t n_reads, uint32_t block_reads,
                        const uint64_t *offs, uint32_t components, uint32_t keep, hipStream_t s);
// One component over n_reads strings of buf: string r is bytes [offs[r] - o, offs[r + 1] - o)
// (offs: n_reads + 1 words; o = *origin, 0 when origin is null: the decoded offsets of a run
// of blocks are relative to the call's first), or with offs null bytes [start[r], start[r] +
// len[r]);
// every position is clamped to buf_bytes, and buf has 8 readable bytes past them.  Block b =
// strings [b block_reads, ...); its digest is ADDED to out[b out_stride] (zeroed by the
// caller).  status (null: none): the pass does nothing unless *status is clear (~0).  Strings
// past kDgLong bytes are taken by a whole workgroup, the others by a quarter-wave.
constexpr uint64_t kDgLong = 2048;
struct DigestArgs {
    const uint8_t *buf;
    uint64_t buf_bytes;
    const uint64_t *offs, *origin;
    const uint32_t *start, *len;
    uint64_t n_reads;
    uint32_t block_reads, bias;  // bias: set by the launcher
    uint64_t *out;
    uint64_t out_stride;         // in 64-bit words
    const unsigned long long *status;
};
void launch_digest(const DigestArgs &a, hipStream_t s);
// decode: block b covers reads [r0[b], r0[b + 1]) (r0: n_blocks + 1 words) of the decoded
// offsets offs; computed[b].n_bases is written, and a block whose bases, or whose digest of a
// component in expected[b].components & checkable, differ sets status to r0[b] << 8 |
// NTC_ERR_DIGEST (lowest block first; a status already set stays).
struct DigestCmpArgs {
    const DigestMetaDev *expected;
    DigestMetaDev *computed;
    const uint64_t *r0;
    uint64_t n_blocks, n_reads;
    const uint64_t *offs;
    uint32_t checkable;
    unsigned long long *status;
};
void launch_digest_compare(const DigestCmpArgs &a, hipStream_t s);

void launch_encode(const EncodeArgs &a, hipStream_t s);
void launch_encode4(const Enc4Args &a, uint64_t total, uint32_t ms_blocks, hipStream_t s,
                    hipEvent_t ev_ms_begin, hipEvent_t ev_ms_end);
// record offsets (rec_offsets[0..n], written here) from the per-wave counts, then records
void launch_emit4(const Enc4Args &a, uint64_t *wave_off, uint64_t *tmp, uint64_t *rec_offsets, uint64_t *out,
                  uint64_t capacity, hipStream_t s);
int ms4_blocks_per_cu();
void launch_debug_gather4(const Enc4Args &a, uint32_t *d_out, uint32_t *s_out, hipStream_t s);
void launch_pair_words(const uint2 *top, uint32_t U, uint16_t *out, hipStream_t s);
void launch_win_words(const uint32_t *bits, uint32_t U, uint32_t *out, hipStream_t s);
// substitution words (encode_core.h subst_clean) into the fourth word of each of the path
// stream's groups; on = false zeroes them.  After the suffix table and the path cover.
void launch_subst_words(const DevIndex &ix, uint4 *pstream, uint64_t groups, bool on, hipStream_t s);
void launch_tab_build(const DevIndex &ix, uint32_t U, uint2 *tab, uint32_t *bits, uint32_t F, uint32_t *fbits,
                      hipStream_t s);
void launch_tile_rows(const uint64_t *offs, uint64_t n_reads, uint32_t *tile_rows, hipStream_t s);
void launch_emit(const EmitArgs &a, hipStream_t s);
void launch_debug_gather(const DebugArgs &a, hipStream_t s);
// decode: per 256-record tile sums (firsts, bases) and their exclusive scans (pfs, pls:
// tiles + 1 words each; pf, pl: tiles words each; tmp: scan_tmp_words(tiles)), then the
// walk kernel, which derives every record's read and output offset itself
void launch_dec_tiles(const uint64_t *recs, uint64_t n, uint64_t *pf, uint64_t *pl, uint64_t *pfs, uint64_t *pls,
                      uint64_t *tmp, hipStream_t s);
void launch_dec_walk(const DecWalkArgs &a, hipStream_t s);
void launch_rank2(const DevIndex &ix, Rank2Chunk *out, hipStream_t s);
// The words of a context's status mailbox (16 words of pinned host memory, written by the last
// kernels of a call and read after the call's own stream sync).  k_status_box fills the first
// four: the call's status, then up to three counts whose meaning is the call's (encode:
// records, entries and records reserved in the overflow pools; decode: reads, bases; FASTQ
// parse: bases kept).  Each side pass owns the words after them.
enum BoxWord {
    kBoxStatus = 0, kBoxA = 1, kBoxB = 2, kBoxC = 3,
    kBoxNxRuns = 4, kBoxNxBases = 5,         // nonacgt.hip k_nx_total: runs found, symbols masked
    kBoxQualStatus = 6, kBoxQualWords = 7,   // quality.hip / qrans.hip: the pass's status, payload words
    kBoxNameStatus = 8, kBoxNameBytes = 9,   // names.hip: the pass's status, payload bytes
    kBoxWeave = 10, kBoxMateCheck = 11,      // pairs.hip k_pair_box: the weave's status, the mate check's
    kBoxPairFirst = 12,                      // pairs.hip k_pair_split: bytes of the first part
    kBoxWindow = 13,                         // window.hip: bytes of the text window
    kBoxQualSmoothed = 14,                   // quality.hip k_q_smooth: bytes replaced (copied from the device counter)
    kBoxWords = 16
};
void launch_status_box(const unsigned long long *status, const uint64_t *a, const uint64_t *b, const uint64_t *c,
                       uint64_t *box, hipStream_t s);
void launch_walk_build(const uint32_t *pred, const uint8_t *code, uint64_t n, WalkStep *a, WalkStep *b,
                       WalkEntry *out, hipStream_t s);
uint64_t scan_tmp_words(uint64_t n);

// Path cover on the device (derived.cpp build_paths, same cover): unitigs of the real
// k-mers, laid out by start node.  Orchestrated by ntc_index_upload.
struct PathArgs {
    const uint2 *rank;       // rank words [4][rwords]
    uint32_t rwords;
    uint32_t n, k;
    const uint8_t *lcs;
    const uint32_t *dummy;   // bit z: node z is a dummy
    const uint32_t *pred;    // inverse-walk predecessor
    const uint8_t *code;     // last character of each node
    const uint32_t *uniq;    // bit z: z's (k-1)-suffix group is {z}
};
// prv[y] = the path predecessor of y, or 0xFFFFFFFF (prv must be preset to all ones)
void launch_path_edges(const PathArgs &a, uint32_t *prv, hipStream_t s);
// list ranking by pointer jumping: st[z] = {start node, distance, min node on the way, 0};
// returns the buffer (a or b) holding the result
uint4 *launch_path_rank(const uint32_t *prv, uint32_t n, uint4 *a, uint4 *b, hipStream_t s);
// unitig linking (derived.cpp link_unitigs): st = the ranking of the unitig edges in prv,
// len[start] = unitig lengths (launch_path_lengths), want preset to all ones, best_pred to
// all ones (64-bit); adds the chosen t -> y edges to prv
void launch_path_link(const PathArgs &a, const uint4 *st, const uint32_t *len, uint32_t *want,
                      unsigned long long *best_pred, uint32_t *prv, hipStream_t s);
// fork blocks after each path end (k >= kForkBlockMinK), after launch_path_place
void launch_path_forks(const PathArgs &a, const uint4 *st, const uint32_t *len, const uint64_t *base,
                       const uint32_t *pos_of_node, const uint4 *pstream, uint32_t *colex_at, hipStream_t s);
// run-length codes into colex_at's node words (encode_core.h uniq_code; n <= kUniqHintMaxN),
// after launch_path_place
void launch_path_hint(uint32_t k, uint64_t tlen, const uint4 *pstream, const uint64_t *puniq, uint32_t *colex_at,
                      hipStream_t s);
// cut every cycle at its smallest node (prv[min] = none); *flag = 1 if any was cut
void launch_path_cut(const PathArgs &a, const uint4 *st, uint32_t *prv, uint32_t *flag, hipStream_t s);
// len[start] = path length (len zeroed first); vals[z] = len + k at starts, else 0;
// *n_paths += number of starts
void launch_path_lengths(const PathArgs &a, const uint4 *st, const uint32_t *prv, uint32_t *len, uint32_t *vals,
                         uint32_t *n_paths, hipStream_t s);
// text, node-end bits, colex_at, pos_of_node, puniq (outputs preset: zeros / all ones)
void launch_path_place(const PathArgs &a, const uint4 *st, const uint32_t *prv, const uint64_t *base,
                       uint32_t *colex_at, uint32_t *pos_of_node, uint4 *pstream, uint64_t *puniq, hipStream_t s);
void scan_excl_u32(const uint32_t *in, uint64_t n, uint64_t *out, uint64_t *tmp, hipStream_t s);
void scan_excl_u64(const uint64_t *in, uint64_t n, uint64_t *out, uint64_t *tmp, hipStream_t s);

}  // namespace ntc
