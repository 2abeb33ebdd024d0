// extern "C" boundary of libntcomp_gpu.so (include/ntcomp_gpu.h, include/ntcomp_host.h).
// Every entry point returns an ntc_status; HIP failures and reference panics become
// status codes plus ntc_last_error(); nothing aborts across the ABI.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <memory>
#include <string>
#include <vector>

#include "../../include/ntcomp_gpu.h"
#include "../../include/ntcomp_codec.h"
#include "../../include/ntcomp_host.h"
#include "codec_params.h"
#include "derived.h"
#include "kernels.h"
#include "nonacgt_core.h"
#include "qrans_core.h"
#include "quality_core.h"
#include "qsmooth_core.h"
#include "names_core.h"
#include "digest_core.h"
#include "bgzf_core.h"
#include "deflate_core.h"
#include "inflate_core.h"
#include "pair_core.h"
#include "window_core.h"
#include "ntc_internal.h"

using namespace ntc;

namespace {

struct DevBuf {
    void *p = nullptr;
    uint64_t bytes = 0;
};

enum CallKind { kNone = 0, kEncode = 1, kDecode = 2 };

}  // namespace

// device workspace slots of a context (grown by ensure, freed with the context)
enum WsSlot {
    WS_D = 0, WS_S, WS_F, WS_R, WS_RECCOUNT, WS_SCANTMP, WS_TILEBASE, WS_TILEROWS,
    WS_STAGE_BASES, WS_STAGE_OFFS, WS_STAGE_RECS, WS_E, WS_DEC_A, WS_DEC_B, WS_DEC_C,
    WS_DEC_D, WS_Q, WS_E3, WS_NE, WS_COUNTER, WS_R2, WS_ED, WS_WAVECNT, WS_PACK_CHUNKS, WS_PACK_META,
    WS_PACK_PAYLOAD, WS_FA_BASES, WS_FA_OFFS, WS_FA_SCAN, WS_ES, WS_OBASE,
    WS_FQ_RAW, WS_FQ_TILES, WS_FQ_NL, WS_FQ_KEPT, WS_PACK_SEGS,
    WS_UNP_PAY, WS_UNP_MARKS, WS_UNP_ST, WS_UNP_VALS, WS_UNP_RECS, WS_UNP_OUT,
    WS_NX_BITS, WS_NX_RUNS, WS_NX_PATCH,
    WS_Q_QUALS, WS_Q_BLOCKS, WS_Q_PAYLOAD, WS_QD_IN, WS_QD_QUALS,
    WS_QR_COUNTS, WS_QR_CUM, WS_QR_SCRATCH, WS_QR_SCAN,
    WS_N_COLS, WS_N_BLOCKS, WS_N_PAYLOAD, WS_ND_IN, WS_ND_COLS, WS_ND_NAMES,
    WS_DG_TABLE, WS_DGD_IN,
    WS_PAIR_IN, WS_PAIR_TAB, WS_PAIR_ST, WS_PAIR_SCAN, WS_PAIR_OUT,
    WS_DF_DESC, WS_DF_TOKENS, WS_DF_STAGE, WS_DF_RES, WS_DF_OUT,
    WS_INF_COMP, WS_INF_DESC, WS_INF_DST, WS_INF_RES,
    WS_BZ_PLAN, WS_BZ_TOKENS, WS_BZ_STAGE, WS_BZ_TEXT, WS_BZ_OFF, WS_BZ_OUT, WS_COUNT
};

// The device index of one upload: freed with the last context that holds it
// (ntc_index_share lets several contexts on one GPU use one copy).
struct IndexMem {
    int device = 0;
    std::vector<void *> ptrs;
    explicit IndexMem(int d) : device(d) {}
    ~IndexMem() {
        (void)hipSetDevice(device);
        for (void *p : ptrs) (void)hipFree(p);
    }
};

namespace {
// Side data handed to the context for the next decode call (ntc_decode_set_*): section metas
// and their payload words.  They leave the context with the call that takes them, which uses
// them once, whether it succeeds or fails.
template <class Meta>
struct Pending {
    std::vector<Meta> metas;
    std::vector<uint64_t> payload;
    bool has = false;
    void clear() { *this = Pending(); }
    bool take(Pending &to) {
        to = has ? std::move(*this) : Pending();
        clear();
        return to.has;
    }
};

// non-ACGT symbols (nonacgt.hip): the policy (0 error, 1 mask, 2 keep), the last encode
// call's counts and runs, the runs waiting for the next decode call (pending.has: any run)
struct NxState {
    int policy = 0;
    uint64_t runs = 0, bases = 0;
    uint64_t cap = 0, cap_hint = 0;  // the run list of the call in flight; what an earlier call needed
    void *d_runs = nullptr;
    std::vector<ntc_nx_run> list;
    Pending<ntc_nx_run> pending;
    uint32_t pending_sub = 0;
    std::vector<ntc_nx_run> pieces;  // the slices of the decode pass in flight (source of an async copy)
    void begin() {  // a host-buffer encode call starts: nothing of the last one is left
        runs = bases = 0;
        list.clear();
    }
};

// quality scores (quality.hip): the mode (0 drop, 1 keep, 2 bin8), the sections the last
// ntc_encode_pack_fastq left in WS_Q_BLOCKS / WS_Q_PAYLOAD, the sections waiting for the
// next FASTA decode call (which then writes FASTQ)
struct QualState {
    int mode = 0;
    int coder = 0;  // option "quality_coder": 0 pack, 1 rans (qrans.hip); coder_last: of those sections
    int coder_last = 0;
    // options "quality_smooth" (0 off, or M) and "quality_smooth_to"; smoothed: bytes the last call replaced
    int smooth = 0, smooth_to = (int)kQsToDefault;
    uint64_t smoothed = 0, smoothed_total = 0;  // (the total: of all calls since "quality_smooth" was last set)
    // a smoothing call in flight: what q_pack prepared and q_finish launches after the encode
    QREncArgs deferred{};
    uint64_t deferred_total = 0;
    uint64_t blocks = 0, words = 0, reads = 0;
    uint32_t block_reads = 0;
    Pending<ntc_qual_meta> pending;
    void begin() { blocks = words = reads = smoothed = 0; }  // an encode call starts: the last call's sections are gone
};

// read names (names.hip): the mode (0 drop, 1 keep, 2 id), the sections the last
// ntc_encode_pack_fastq left in WS_N_BLOCKS / WS_N_PAYLOAD, the sections waiting for the
// next FASTA decode call (which then writes the names instead of seq.N)
struct NameState {
    int mode = 0;
    uint64_t blocks = 0, bytes = 0;
    const uint32_t *d_start = nullptr, *d_len = nullptr;  // the name spans of the names pass in flight
    Pending<ntc_name_meta> pending;
    void begin() { blocks = bytes = 0; }  // an encode call starts: the last call's sections are gone
};

// content digests (digest.hip): the option (0 off, 1 on), the table the last
// ntc_encode_pack_* call left in WS_DG_TABLE, the expected digests waiting for the next
// FASTA decode call, and what the last such call computed (WS_DGD_IN holds both on the device)
struct DigestState {
    int opt = 0;
    uint64_t blocks = 0;
    Pending<ntc_digest_meta> pending;  // (no payload)
    std::vector<ntc_digest_meta> expected, computed;
    uint32_t checkable = 0;  // the components that call could compute
    void begin() { blocks = 0; }  // an encode call starts: the last call's digests are gone
};

// paired-end reads (pairs.hip): the option (0 off, 1 pairs with the mate check, 2 pairs
// without it); whether the last text decode was split, and the bytes of its first part
struct PairState {
    int mode = 0;
    bool valid = false;
    uint64_t first = 0;
};

// deflate on the device (deflate.hip): the option "gpu_deflate"; the chunk and stream lists of the
// call in flight (the source of its upload) and the members the last encode_pack call left
struct DeflateState {
    int opt = 0;
    std::vector<DfChunkDesc> chunks;
    std::vector<DfStreamDesc> streams;
    std::vector<uint64_t> dev_off_len;  // as the device wrote them, the total behind them
    std::vector<uint64_t> members;      // 4 pairs (offset, bytes) per block of the last call
    void begin() { members.clear(); }   // an encode call starts: the last call's members are gone
};

// BGZF output (bgzf.hip): the options "bgzf_text" (a text decode call leaves BGZF members in
// place of its text) and "bgzf_workgroups" (k_bgzf_chunks' grid, 0: two per CU); the member
// table and the counts of the last call that made members (ntc_bgzf_last)
struct BgzfState {
    int opt = 0;
    int workgroups = 0;
    std::vector<BgzfMember> members;
    uint64_t counts[7] = {0, 0, 0, 0, 0, 0, 0};  // members, chunks, text bytes, bytes, chunks stored / Huffman / with matches
    double seconds = 0;  // inside the plan, the coder and the members' copy
    void begin() {
        members.clear();
        for (uint64_t &c : counts) c = 0;
        seconds = 0;
    }
};

// the text window of the next ntc_decode_fasta / _unpacked (ntc_decode_set_window): pending
// like the side data above, gone after that call whether it succeeds or fails
struct WindowState {
    bool has_pending = false;
    uint64_t first = 0, count = 0;
};
}  // namespace

struct ntc_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = true;
    std::string err;
    // index
    bool has_index = false;
    DevIndex dix{};
    std::shared_ptr<IndexMem> index_mem;
    uint64_t index_bytes = 0;
    // workspace buffers (grown, never shrunk)
    DevBuf ws[WS_COUNT];
    unsigned long long *d_status = nullptr;
    // status mailbox in pinned host memory (kernels.h BoxWord names its words), written by the
    // last kernels of a device call, so *_status() is one stream sync instead of D2H copies
    uint64_t *h_box = nullptr;
    bool box_valid = false;
    // the records of the last ntc_unpack_streams (in WS_UNP_RECS) and their read / base counts
    uint64_t *unp_d_recs = nullptr;
    uint64_t unp_recs = 0, unp_reads = 0, unp_bases = 0;
    uint64_t unp_path[3] = {0, 0, 0};  // its Rice streams flagged not-simple, serial; segments run through
    // last call
    CallKind last = kNone;
    uint64_t last_n = 0;           // reads (encode) / records (decode)
    uint64_t *last_out_offs = nullptr;
    uint64_t last_units = 0;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    int encode_variant = 4;
    int last_variant = 0;
    int num_cus = 0;
    Enc4Args last4{};
    // the last v4 encode's arguments: a call that ran out of an overflow pool is re-run
    // with grown pools when its status is read (read_status)
    struct {
        const uint8_t *bases;
        const uint64_t *offs;
        uint64_t n_reads, total_bases, cap;
        uint64_t *rec_out, *rec_offs;
    } call4{};
    uint32_t ent_slots_opt = 0;     // secondary entry slots per read (0: auto, 16 with joint runs, else 4)
    double epool_per_read = 4.0;    // overflow pools: a floor per read (the test hook pool_per_read sets it)
    double rpool_per_read = 1.0;
    double epool_per_base = 0.0;    // and what the last call's reads reserved per base (learn_pool_rates)
    double rpool_per_base = 0.0;
    uint64_t spill_reruns = 0;      // calls re-run with grown pools
    uint32_t tab_u_opt = 0;  // suffix-table depth for the next upload (0 = default_tab_u)
    int tab_u_fallback = 0;  // last upload: the default depth did not fit, U = 14 was used
    int pair_bytes_opt = 1;  // build the SCAN pair bytes at the next upload (0: bitmap tests, A/B)
    int filter_opt = -1;     // SCAN pre-filter at the next upload: -1 auto (off when saturated), 0 off, 1 on
    int64_t filter_density_ppm = -1;  // presence density of the filter level at the last upload
    int joint_opt = -1;      // joint path runs at the next upload: -1 auto (fragmented path cover), 0 off, 1 on
    int path_link_opt = path_link_on() ? 1 : 0;  // path cover: unitigs linked across branches (default) or not
    int win_opt = -1;        // SCAN window words at the next upload: -1 auto (U >= 4), 0 off, 1 on
    int subst_opt = subst_on() ? -1 : 0;  // substitution words at the next upload: -1 auto (the build without
                                               // joint runs, path positions in the table, U >= 4), 0 zeroed
    int subst_built = 0;     // the index in use carries substitution words
    int uniq_hint_opt = uniq_hint_on() ? -1 : 0;  // run-length codes in colex_at at the next upload: -1 auto
                                                  // (n <= kUniqHintMaxN), 0 none
    int decode_only_opt = 0;  // the next upload builds only what decode needs (walk table): no path
                              // cover, suffix table or SCAN words; encode calls then fail
    bool index_decode_only = false;  // the index in use was uploaded that way
    int ext2_opt = 0;        // build the two-character rank chunks at the next upload (A/B option: 1 measured
                             // slower -- 8 B/node from HBM against 1 B/node of Infinity-Cache-resident rank words)
    uint64_t n_paths = 0, path_text_len = 0;
    int64_t upload_host_us = 0, upload_total_us = 0;  // last ntc_index_upload: host derive / total
    uint64_t max_pass_bases = 1ULL << 30;  // host-buffer calls split into device passes of at most this
    double last_pack_ms = 0;               // last ntc_pack_blocks_device: both packer kernels
    NxState nx;
    QualState qual;
    NameState names;
    DigestState dig;
    PairState pair;
    WindowState win;
    DeflateState df;
    BgzfState bz;
    int discard_text = 0;  // option "discard_text": a FASTA decode call formats its text and leaves it on the device
    FastqArgs fq_last{};              // the last GPU FASTQ parse (run again when the run list was short)
    hipEvent_t pack_ev[3] = {nullptr, nullptr, nullptr};
};

namespace {

// work queue heads (kernels.hip WaveQueue: 8, 64 B apart), then the two pool counters
// (kPoolCntE, kPoolCntR: words 64 and 72)
constexpr uint64_t kCounterBytes = 8 * 64 + 2 * 64;

#define HIP_TRY(ctx, expr)                                                                   \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) {                                                              \
            (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                   \
            return NTC_ERR_HIP;                                                              \
        }                                                                                    \
    } while (0)

int set_err(ntc_ctx *ctx, int code, const std::string &msg) {
    if (ctx) ctx->err = msg;
    return code;
}

int ensure(ntc_ctx *ctx, int slot, uint64_t bytes, void **out) {
    DevBuf &b = ctx->ws[slot];
    if (bytes == 0) bytes = 64;
    if (b.bytes < bytes) {
        if (b.p) {
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            HIP_TRY(ctx, hipFree(b.p));
            b.p = nullptr;
            b.bytes = 0;
        }
        uint64_t want = bytes + bytes / 8;  // headroom for slightly larger next calls
        if (hipMalloc(&b.p, want) != hipSuccess) {
            (void)hipGetLastError();
            b.p = nullptr;
            want = bytes;  // no headroom when memory is short
            if (hipMalloc(&b.p, want) != hipSuccess) {
                (void)hipGetLastError();
                b.p = nullptr;
                size_t fr = 0, tot = 0;
                (void)hipMemGetInfo(&fr, &tot);
                return set_err(ctx, NTC_ERR_CAPACITY,
                               "device workspace of " + std::to_string(bytes) + " bytes does not fit (" +
                                   std::to_string(fr) + " bytes free): split the batch");
            }
        }
        b.bytes = want;
    }
    *out = b.p;
    return NTC_OK;
}
// a word of the status mailbox, after the stream sync that its writer's call ends with
inline uint64_t box(const ntc_ctx *ctx, BoxWord w) { return ((volatile uint64_t *)ctx->h_box)[w]; }

// an encode call starts, or failed: no side data of an earlier call is left to fetch
inline void side_begin(ntc_ctx *ctx) {
    ctx->nx.begin();
    ctx->qual.begin();
    ctx->names.begin();
    ctx->dig.begin();
    ctx->df.begin();
}

const char *status_name(int code) {
    switch (code) {
    case NTC_ERR_INVALID_BASE: return "invalid base (non-ACGT or absent from the index)";
    case NTC_ERR_EMPTY_READ: return "empty read (EncodeError)";
    case NTC_ERR_LENGTH: return "match length >= 2^24";
    case NTC_ERR_CAPACITY: return "output capacity exceeded";
    case NTC_ERR_FORMAT: return "malformed input";
    case NTC_ERR_REFERENCE_PANIC: return "short record longer than k (the reference panics, encode.rs:151-152)";
    case NTC_ERR_DIGEST: return "content digest of the block differs; its first read";
    default: return "error";
    }
}

// Scratch layout for n_reads reads: either per-tile bases (tile_base, device pointer)
// or uniform rows per tile.
struct Layout {
    const uint64_t *d_tile_base = nullptr;
    uint64_t rows_uniform = 0;
    uint64_t total_rows = 0;
};

int alloc_scratch(ntc_ctx *ctx, uint64_t n_reads, uint64_t total_rows, EncodeArgs &a) {
    void *p;
    int rc;
    const uint64_t slots = total_rows * 64;
    if ((rc = ensure(ctx, WS_D, slots, &p))) return rc;
    a.D = (uint8_t *)p;
    if ((rc = ensure(ctx, WS_S, slots * 4, &p))) return rc;
    a.S = (uint32_t *)p;
    if ((rc = ensure(ctx, WS_F, (total_rows / 32 + 1) * 64 * 4, &p))) return rc;
    a.F = (uint32_t *)p;
    if ((rc = ensure(ctx, WS_R, slots * 8, &p))) return rc;
    a.R = (uint64_t *)p;
    if ((rc = ensure(ctx, WS_RECCOUNT, (n_reads + 1) * 4, &p))) return rc;
    a.rec_count = (uint32_t *)p;
    return NTC_OK;
}

// overflow pool indices are 32-bit (MsLaneT::ob, rbase)
constexpr uint64_t kPoolMax = 0xFFFFFFF0ull;

uint32_t ent_slots(const ntc_ctx *ctx) {
    if (ctx->ent_slots_opt) return ctx->ent_slots_opt;
    // entries per read past the dense 4 (tests/emu NTC_EMU_SPILL, 1 % errors): random genome
    // k = 91 reads rarely spill (6 %, 0.07 % past 8); a strain collection with joint runs and
    // fork hops spills on 98 % of reads.  With the linked path cover (round 6) S91's reads
    // have fewer run entries: 16 secondary slots measured 131.2-131.7 Gbases/s against
    // 129.9-130.9 with 20 (3 runs each, one box); the overflow pool takes the rest
    return ctx->has_index && ctx->dix.joint ? 16u : 4u;
}

// v4: pack -> persistent MS -> parse -> scan -> emit, all in position space.
// total_bases = offs[n] - offs[0] (known to the caller).
int encode4_impl(ntc_ctx *ctx, const uint8_t *d_bases, const uint64_t *d_offs, uint64_t n_reads,
                 uint64_t total_bases, uint64_t *d_rec_out, uint64_t cap, uint64_t *d_rec_offs) {
    if (ctx->index_decode_only)
        return set_err(ctx, NTC_ERR_NO_INDEX, "the index was uploaded for decode only (ctx option decode_only)");
    // k_ms4's query-word cache names 16-byte pairs of the 2-bit stream by a 32-bit index
    // (encode_core.h NTC_QCACHE): a call stays below 2^38 bases (256 Gi, more than HBM holds)
    if (total_bases >= (1ull << 38)) return set_err(ctx, NTC_ERR_CAPACITY, "2^38 bases or more in one call: split the batch");
    Enc4Args a{};
    a.ix = ctx->dix;
    a.bases = d_bases;
    a.offs = d_offs;
    a.n_reads = n_reads;
    a.status = ctx->d_status;
    void *p;
    int rc;
    ctx->call4 = {d_bases, d_offs, n_reads, total_bases, cap, d_rec_out, d_rec_offs};
    // Workspace by need: per read, 4 dense + S secondary entry slots, 8 dense record slots;
    // the rest of a read's entries / records go to overflow pools sized from what earlier
    // calls reserved (a call that runs out is re-run with the pools grown, read_status).
    const uint32_t S = ent_slots(ctx);
    // A read never holds more entries or records than it has positions, so this call's bases
    // bound both pools whatever rate an earlier call (e.g. one of long reads) left behind.
    const uint64_t pos_cap = total_bases + 4 * n_reads + 4096;  // + reservations rounded to 4-entry groups
    auto pool_size = [&](double per_read, double per_base) {
        const double want = std::max(per_read * (double)n_reads, per_base * (double)total_bases);
        return std::min<uint64_t>(std::min<uint64_t>((uint64_t)want + 4096, pos_cap), kPoolMax);
    };
    const uint64_t pcap = pool_size(ctx->epool_per_read, ctx->epool_per_base);
    const uint64_t rcap = pool_size(ctx->rpool_per_read, ctx->rpool_per_base);
    if ((rc = ensure(ctx, WS_Q, (total_bases / 32 + 4) * 8, &p))) return rc;
    a.Q = (uint64_t *)p;
    if ((rc = ensure(ctx, WS_ES, (n_reads + 1) * S * sizeof(Entry), &p))) return rc;
    a.Es = (Entry *)p;
    a.S = S;
    if ((rc = ensure(ctx, WS_E3, pcap * sizeof(Entry), &p))) return rc;
    a.Ep = (Entry *)p;
    a.pcap = pcap;
    if ((rc = ensure(ctx, WS_OBASE, (n_reads + 1) * 8, &p))) return rc;
    a.obase = (uint32_t *)p;
    a.rbase = a.obase + (n_reads + 1);
    if ((rc = ensure(ctx, WS_ED, (n_reads + 1) * kEntSlot * sizeof(Entry), &p))) return rc;
    a.Ed = (Entry *)p;
    if ((rc = ensure(ctx, WS_NE, (n_reads + 1) * 4, &p))) return rc;
    a.ne = (uint32_t *)p;
    if ((rc = ensure(ctx, WS_R, rcap * 8, &p))) return rc;
    a.R = (uint64_t *)p;
    a.rcap = rcap;
    if ((rc = ensure(ctx, WS_R2, (n_reads + 1) * kRecSlot * 8, &p))) return rc;
    a.R2 = (uint64_t *)p;
    if ((rc = ensure(ctx, WS_RECCOUNT, (n_reads + 1) * 4, &p))) return rc;
    a.rec_count = (uint32_t *)p;
    const uint64_t waves = (n_reads + 63) / 64;
    if ((rc = ensure(ctx, WS_WAVECNT, (waves + 1) * 4 + (waves + 2) * 8 + 8, &p))) return rc;
    a.wave_cnt = (uint32_t *)p;
    uint64_t *wave_off = (uint64_t *)(((uintptr_t)(a.wave_cnt + waves + 1) + 7) & ~(uintptr_t)7);
    if ((rc = ensure(ctx, WS_COUNTER, kCounterBytes, &p))) return rc;
    a.counter = (unsigned long long *)p;
    void *tmp;
    if ((rc = ensure(ctx, WS_SCANTMP, scan_tmp_words(n_reads + 1) * 8, &tmp))) return rc;
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_status, 0xFF, 8, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(a.counter, 0, kCounterBytes, ctx->stream));
    ctx->box_valid = false;
    ctx->last = kEncode;
    ctx->last_variant = 4;
    ctx->last_n = n_reads;
    ctx->last_out_offs = d_rec_offs;
    ctx->last_units = total_bases;
    ctx->last4 = a;
    HIP_TRY(ctx, hipEventRecord(ctx->ev[0], ctx->stream));
    if (n_reads == 0) {
        HIP_TRY(ctx, hipMemsetAsync(d_rec_offs, 0, 8, ctx->stream));
        for (int i = 1; i < 4; i++) HIP_TRY(ctx, hipEventRecord(ctx->ev[i], ctx->stream));
        return NTC_OK;
    }
    static int bpc = 0;
    if (!bpc) bpc = ms4_blocks_per_cu();
    launch_encode4(a, total_bases, (uint32_t)(ctx->num_cus * bpc), ctx->stream, ctx->ev[3], ctx->ev[1]);
    HIP_TRY(ctx, hipGetLastError());
    launch_emit4(a, wave_off, (uint64_t *)tmp, d_rec_offs, d_rec_out, cap, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ctx->ev[2], ctx->stream));
    launch_status_box(ctx->d_status, d_rec_offs + n_reads, (const uint64_t *)(a.counter + kPoolCntE),
                      (const uint64_t *)(a.counter + kPoolCntR), ctx->h_box, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    ctx->box_valid = true;
    return NTC_OK;
}

// Pool rates for the next call: what this call's reads reserved (plus a quarter) per input
// base.  Taken from the latest call alone and per base, not per read, so a batch of long
// reads does not inflate the pools of later batches of short ones.
void learn_pool_rates(ntc_ctx *ctx, uint64_t cnt_e, uint64_t cnt_r) {
    const double b = (double)(ctx->call4.total_bases ? ctx->call4.total_bases : 1);
    ctx->epool_per_base = 1.25 * (double)cnt_e / b;
    ctx->rpool_per_base = 1.25 * (double)cnt_r / b;
}

int encode_impl(ntc_ctx *ctx, const uint8_t *d_bases, const uint64_t *d_offs, uint64_t n_reads,
                const Layout &lay, uint64_t *d_rec_out, uint64_t cap, uint64_t *d_rec_offs,
                uint64_t units) {
    if (!ctx->has_index) return set_err(ctx, NTC_ERR_NO_INDEX, "no index uploaded");
    if (ctx->index_decode_only)
        return set_err(ctx, NTC_ERR_NO_INDEX, "the index was uploaded for decode only (ctx option decode_only)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ctx->last_variant = ctx->encode_variant;
    EncodeArgs a{};
    a.ix = ctx->dix;
    a.bases = d_bases;
    a.offs = d_offs;
    a.n_reads = n_reads;
    a.tile_base = lay.d_tile_base;
    a.rows_uniform = lay.rows_uniform;
    a.status = ctx->d_status;
    int rc = alloc_scratch(ctx, n_reads, lay.total_rows, a);
    if (rc) return rc;
    void *tmp;
    if ((rc = ensure(ctx, WS_SCANTMP, scan_tmp_words(n_reads + 1) * 8, &tmp))) return rc;
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_status, 0xFF, 8, ctx->stream));
    ctx->box_valid = false;
    ctx->last = kEncode;
    ctx->last_n = n_reads;
    ctx->last_out_offs = d_rec_offs;
    ctx->last_units = units;
    if (n_reads == 0) {
        HIP_TRY(ctx, hipMemsetAsync(d_rec_offs, 0, 8, ctx->stream));
        for (int i = 0; i < 3; i++) HIP_TRY(ctx, hipEventRecord(ctx->ev[i], ctx->stream));
        return NTC_OK;
    }
    HIP_TRY(ctx, hipEventRecord(ctx->ev[0], ctx->stream));
    launch_encode(a, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ctx->ev[1], ctx->stream));
    scan_excl_u32(a.rec_count, n_reads, d_rec_offs, (uint64_t *)tmp, ctx->stream);
    EmitArgs e{};
    e.R = a.R;
    e.tile_base = lay.d_tile_base;
    e.rows_uniform = lay.rows_uniform;
    e.rec_count = a.rec_count;
    e.rec_offsets = d_rec_offs;
    e.n_reads = n_reads;
    e.out = d_rec_out;
    e.capacity = cap;
    e.status = ctx->d_status;
    launch_emit(e, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ctx->ev[2], ctx->stream));
    return NTC_OK;
}

// A v4 encode that ran out of an overflow pool (status kStatusRegrow): the pool counters
// hold what every read reserved, so the pools grow to that (plus a quarter, remembered per
// read for later calls) and the call runs again on the same inputs.
int regrow_and_rerun(ntc_ctx *ctx) {
    uint64_t cnt[2] = {0, 0};
    HIP_TRY(ctx, hipMemcpy(&cnt[0], ctx->last4.counter + kPoolCntE, 8, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(&cnt[1], ctx->last4.counter + kPoolCntR, 8, hipMemcpyDeviceToHost));
    learn_pool_rates(ctx, cnt[0], cnt[1]);
    if ((cnt[0] > kPoolMax || cnt[1] > kPoolMax))
        return set_err(ctx, NTC_ERR_CAPACITY, "entry / record overflow past 2^32 slots: split the batch");
    ctx->spill_reruns++;
    const auto &c = ctx->call4;
    return encode4_impl(ctx, c.bases, c.offs, c.n_reads, c.total_bases, c.rec_out, c.cap, c.rec_offs);
}

int read_status(ntc_ctx *ctx, int64_t *bad_index) {
    for (int attempt = 0;; attempt++) {
        unsigned long long st = 0;
        if (ctx->box_valid) {  // the call's mailbox (k_status_box): one stream sync
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            st = box(ctx, kBoxStatus);
        } else {
            HIP_TRY(ctx, hipMemcpyAsync(&st, ctx->d_status, 8, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        }
        if (st == ~0ULL) {
            if (bad_index) *bad_index = -1;
            if (ctx->box_valid && ctx->last == kEncode && ctx->last_variant == 4)
                learn_pool_rates(ctx, box(ctx, kBoxB), box(ctx, kBoxC));
            return NTC_OK;
        }
        if (st == kStatusRegrow) {
            // up to 4 re-runs: the first call on a context learns the entry pool (the parse
            // is skipped while entries overflow), then the record pool; a 10 M-read call on a
            // 177 M-node collection (L31, profiles/round5/big_point_*) ran out after two
            if (ctx->last == kEncode && ctx->last_variant == 4 && attempt < 4) {
                const int rc = regrow_and_rerun(ctx);
                if (rc) return rc;
                continue;
            }
            if (bad_index) *bad_index = -1;
            return set_err(ctx, NTC_ERR_CAPACITY, "entry / record overflow pool exhausted after re-runs");
        }
        int code = (int)(st & 0xFF);
        int64_t idx = (int64_t)(st >> 8);
        if (bad_index) *bad_index = idx;
        char buf[160];
        std::snprintf(buf, sizeof(buf), "%s at index %lld", status_name(code), (long long)idx);
        ctx->err = buf;
        return code;
    }
}

// A decode-side pass may have set the call's status after the walk filled the mailbox: fill it
// again (same counts), so the call's one sync still reads the final status.
int rebox_decode(ntc_ctx *ctx) {
    if (ctx->box_valid && ctx->last == kDecode)
        launch_status_box(ctx->d_status, ctx->last_out_offs + ctx->last_n,
                          ctx->last_out_offs + (ctx->last_n + 1) + ctx->last_n, nullptr, ctx->h_box, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    return NTC_OK;
}

// ---- non-ACGT symbols (nonacgt.hip) ---------------------------------------------------
// Before an encode of staged bases (the library's own, writable copy): flag, list the runs
// (policy keep), substitute.  Asynchronous; the counts reach the host in mailbox words
// kBoxNxRuns and kBoxNxBases with the encode call's own status sync (nx_collect).  Policy 0
// launches nothing.
int nx_mask(ntc_ctx *ctx, uint8_t *d_bases, const uint64_t *d_offs, uint64_t n_reads, uint64_t total) {
    ctx->nx.cap = 0;
    if (ctx->nx.policy == 0) return NTC_OK;
    ctx->h_box[kBoxNxRuns] = ctx->h_box[kBoxNxBases] = 0;  // (the last call's kernels are done: every encode call ends synchronised)
    if (n_reads == 0) return NTC_OK;
    if (!ctx->has_index) return set_err(ctx, NTC_ERR_NO_INDEX, "no index uploaded");
    const uint32_t sub = nx_substitute(ctx->dix.absent);
    if (!sub) return set_err(ctx, NTC_ERR_INVALID_BASE, "the index contains none of A, C, G, T");
    // a run's pos and len are 32-bit: a pass below 2^32 bases cannot overflow them
    if (total >= (1ull << 32))
        return set_err(ctx, NTC_ERR_CAPACITY, "non_acgt mask / keep: 2^32 bases or more in one device pass: split the batch");
    NxArgs a{};
    a.bases = d_bases;
    a.offs = d_offs;
    a.n_reads = n_reads;
    a.total = total;
    a.n_words = nx_words(total);
    const uint64_t W = a.n_words;
    void *p, *tmp;
    int rc;
    // M, S, E, soff, eoff (W + 1 words each, 8-byte aligned), counts, then cnt_s, cnt_e
    if ((rc = ensure(ctx, WS_NX_BITS, (5 * (W + 1) + 2) * 8 + 2 * (W + 1) * 4, &p))) return rc;
    a.M = (uint64_t *)p;
    a.S = a.M + (W + 1);
    a.E = a.S + (W + 1);
    a.soff = a.E + (W + 1);
    a.eoff = a.soff + (W + 1);
    a.counts = a.eoff + (W + 1);
    a.cnt_s = (uint32_t *)(a.counts + 2);
    a.cnt_e = a.cnt_s + (W + 1);
    if ((rc = ensure(ctx, WS_SCANTMP, scan_tmp_words(std::max(W, n_reads) + 1) * 8, &tmp))) return rc;
    if (ctx->nx.policy == 2) {
        // room for a run per 16 bases, or what an earlier call needed; a call that finds
        // more is staged and run again with the exact room (nx_collect)
        ctx->nx.cap = std::min<uint64_t>(std::max<uint64_t>(total / 16 + 4096, ctx->nx.cap_hint), total + 1);
        if ((rc = ensure(ctx, WS_NX_RUNS, ctx->nx.cap * sizeof(ntc_nx_run), &p))) return rc;
        ctx->nx.d_runs = p;
        a.runs = (NxRun *)p;
        a.run_cap = ctx->nx.cap;
    }
    a.box = ctx->h_box;
    a.sub = sub;
    a.status = ctx->d_status;
    launch_nx_mask(a, (uint64_t *)tmp, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    return NTC_OK;
}

// After the encode call's status sync: the counts, and under policy keep the runs, appended
// to the context's list with read_base added.  *again: the list was too short -- the caller
// stages the bases afresh (they are masked by now) and runs the call again.
int nx_collect(ntc_ctx *ctx, uint64_t read_base, bool *again) {
    *again = false;
    if (ctx->nx.policy == 0) return NTC_OK;
    const uint64_t n = box(ctx, kBoxNxRuns), nb = box(ctx, kBoxNxBases);
    if (ctx->nx.policy == 2 && n > ctx->nx.cap) {
        ctx->nx.cap_hint = n + n / 4;
        *again = true;
        return NTC_OK;
    }
    ctx->nx.runs += n;
    ctx->nx.bases += nb;
    if (ctx->nx.policy != 2 || n == 0) return NTC_OK;
    const size_t at = ctx->nx.list.size();
    ctx->nx.list.resize(at + n);
    HIP_TRY(ctx, hipMemcpy(ctx->nx.list.data() + at, ctx->nx.d_runs, n * sizeof(ntc_nx_run), hipMemcpyDeviceToHost));
    if (read_base)
        for (size_t i = at; i < at + n; i++) ctx->nx.list[i].read += read_base;
    return NTC_OK;
}

// Decode side: the pending runs with read in [r0, r0 + n_reads) over that pass's decoded
// bases and offsets (read offsets from 0), long runs cut into slices for k_nx_patch; then
// the status mailbox again, as the patch may have set the status.
int nx_patch(ntc_ctx *ctx, const std::vector<ntc_nx_run> &runs, uint32_t sub, uint64_t r0, uint64_t n_reads,
             uint8_t *d_bases, const uint64_t *d_offs) {
    constexpr uint32_t kSlice = 1u << 16;
    auto lo = std::lower_bound(runs.begin(), runs.end(), r0,
                               [](const ntc_nx_run &x, uint64_t v) { return x.read < v; });
    auto hi = std::lower_bound(lo, runs.end(), r0 + n_reads, [](const ntc_nx_run &x, uint64_t v) { return x.read < v; });
    if (lo == hi) return NTC_OK;
    std::vector<ntc_nx_run> &pc = ctx->nx.pieces;
    pc.clear();
    pc.reserve((size_t)(hi - lo));
    for (auto it = lo; it != hi; ++it) {
        ntc_nx_run r = *it;
        r.read -= r0;
        // a slice must stay a run that fits, so pos + len overflowing 32 bits is cut to fail whole
        if ((uint64_t)r.pos + r.len > 0xFFFFFFFFull || r.len <= kSlice) {
            pc.push_back(r);
            continue;
        }
        for (uint32_t done = 0; done < it->len; done += kSlice) {
            r.pos = it->pos + done;
            r.len = std::min(kSlice, it->len - done);
            pc.push_back(r);
        }
    }
    void *d_pc;
    int rc;
    if ((rc = ensure(ctx, WS_NX_PATCH, pc.size() * sizeof(ntc_nx_run), &d_pc))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(d_pc, pc.data(), pc.size() * sizeof(ntc_nx_run), hipMemcpyHostToDevice, ctx->stream));
    NxPatchArgs a{};
    a.runs = (const NxRun *)d_pc;
    a.n = pc.size();
    a.bases = d_bases;
    a.offs = d_offs;
    a.n_reads = n_reads;
    a.sub = sub;
    a.status = ctx->d_status;
    launch_nx_patch(a, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    return rebox_decode(ctx);
}

// ---- quality scores (quality.hip) -------------------------------------------------------
// After a GPU FASTQ parse (the text, its newline table and the read offsets are in HBM):
// gather, alphabets, pack.  Asynchronous: the pass has a status word of its own (d_status is
// preset again by the encode that follows), which reaches the host with the payload's size
// in mailbox words kBoxQualStatus and kBoxQualWords at the encode call's own status sync
// (q_collect).  Mode 0 returns before anything is launched.
//
// defer (option "quality_smooth"): only k_q_gather runs here, and q_finish does the rest once
// the encode has its final records; the workspace of both halves is ensured here.
int q_pack(ntc_ctx *ctx, const uint64_t *d_offs, uint64_t n_reads, uint64_t total, uint32_t block_reads, bool defer) {
    if (ctx->qual.mode == 0 || n_reads == 0) return NTC_OK;
    const uint64_t nb = (n_reads + block_reads - 1) / block_reads;
    void *quals, *blk, *pay;
    int rc;
    if ((rc = ensure(ctx, WS_Q_QUALS, total + 64, &quals))) return rc;
    // the status word, the presence maps (16 B per block), the blocks and their totals
    if ((rc = ensure(ctx, WS_Q_BLOCKS, 64 + nb * 16 + (nb + 1) * sizeof(QBlock), &blk))) return rc;
    const bool rans = ctx->qual.coder == 1;
    if ((rc = ensure(ctx, WS_Q_PAYLOAD, rans ? qr_payload_bytes_max(total, nb) : q_payload_words_max(total, nb) * 8, &pay)))
        return rc;
    const FastqArgs &f = ctx->fq_last;
    QEncArgs a{};
    a.raw = f.raw;
    a.n_raw = f.n_raw;
    a.nl = f.nl;
    a.n_nl_p = f.tile_base + fastq_tiles(f.n_raw);
    a.offs = d_offs;
    a.n_reads = n_reads;
    a.n_blocks = nb;
    a.block_reads = block_reads;
    a.mode = (uint32_t)ctx->qual.mode;
    a.quals = (uint8_t *)quals;
    a.status = (unsigned long long *)blk;
    a.pres = (uint32_t *)((uint8_t *)blk + 64);
    a.blocks = (QBlock *)((uint8_t *)blk + 64 + nb * 16);
    a.payload = (uint64_t *)pay;
    a.box = ctx->h_box;
    ctx->h_box[kBoxQualStatus] = ~0ull;  // (the last call's kernels are done: every encode call ends synchronised)
    ctx->h_box[kBoxQualWords] = 0;
    ctx->h_box[kBoxQualSmoothed] = 0;
    ctx->qual.coder_last = ctx->qual.coder;
    if (defer) {
        ctx->qual.deferred = QREncArgs{};
        ctx->qual.deferred.q = a;
        ctx->qual.deferred_total = total;
        launch_quality_lines(a, ctx->stream);
        HIP_TRY(ctx, hipGetLastError());
        if (!rans) return NTC_OK;
    } else if (!rans) {
        launch_quality_pack(a, total, ctx->stream);
        HIP_TRY(ctx, hipGetLastError());
        return NTC_OK;
    }
    // coder 1: counts, cumulative rows, a scratch slot per span, the span sizes and their scan
    const uint64_t S = qr_spans_max(total, nb);
    void *cnt, *cum, *scr, *scan;
    if ((rc = ensure(ctx, WS_QR_COUNTS, nb * kQRCountStride * 4, &cnt))) return rc;
    if ((rc = ensure(ctx, WS_QR_CUM, nb * kQRCumStride * 2, &cum))) return rc;
    if ((rc = ensure(ctx, WS_QR_SCRATCH, S * kQRSlot + 64, &scr))) return rc;
    if ((rc = ensure(ctx, WS_QR_SCAN, (2 * (S + 1) + scan_tmp_words(S)) * 8, &scan))) return rc;
    QREncArgs ra{};
    ra.q = a;
    ra.counts = (uint32_t *)cnt;
    ra.cum = (uint16_t *)cum;
    ra.scratch = (uint8_t *)scr;
    ra.sizes = (uint64_t *)scan;
    ra.offs = ra.sizes + (S + 1);
    ra.tmp = ra.offs + (S + 1);
    ra.spans_max = S;
    if (defer) {
        ctx->qual.deferred = ra;
        return NTC_OK;
    }
    launch_quality_gather(a, ctx->stream);
    launch_quality_rans(ra, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    return NTC_OK;
}
int dg_add(ntc_ctx *ctx, uint32_t c, const void *buf, uint64_t buf_bytes, const uint64_t *offs, const uint32_t *start,
           const uint32_t *len, uint64_t n_reads, uint32_t block_reads);
// The rest of a deferred quality pass, after encode_pack_staged (which ended synchronised, its
// final records in WS_STAGE_RECS, their offsets behind d_offs).  encoded: the rule, the
// presence maps, the alphabets, the coder and the qual digest; otherwise only k_q_alpha, so
// that the gather's verdict reaches the mailbox.  Ends with the pass's own sync.
int q_finish(ntc_ctx *ctx, bool encoded, const uint64_t *d_offs, uint64_t n_reads, uint64_t total, uint32_t block_reads,
             uint32_t dg) {
    const QREncArgs &ra = ctx->qual.deferred;
    if (encoded) {
        QSmoothArgs sa{};
        sa.q = ra.q;
        sa.recs = (const uint64_t *)ctx->ws[WS_STAGE_RECS].p;
        sa.roffs = d_offs + (n_reads + 1);
        sa.m = (uint32_t)ctx->qual.smooth;
        sa.to = (uint32_t)ctx->qual.smooth_to;
        sa.count = ra.q.status + 1;  // (the status word has 64 bytes to itself)
        launch_quality_smooth(sa, ctx->stream);
        HIP_TRY(ctx, hipMemcpyAsync(ctx->h_box + kBoxQualSmoothed, sa.count, 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    launch_quality_alpha(ra.q, ctx->stream);
    if (encoded && ctx->qual.coder_last == 1) launch_quality_rans(ra, ctx->stream);
    else if (encoded) launch_quality_spans(ra.q, ctx->qual.deferred_total, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    int rc;
    if (encoded && (dg & kDgQual) &&
        (rc = dg_add(ctx, 2, ra.q.quals, total, d_offs, nullptr, nullptr, n_reads, block_reads)))
        return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return NTC_OK;
}
// After the encode call's sync: the quality pass's verdict.  A read it refused fails the call.
int q_collect(ntc_ctx *ctx, uint64_t n_reads, uint32_t block_reads, int64_t *bad_read) {
    if (ctx->qual.mode == 0 || n_reads == 0) return NTC_OK;
    const uint64_t st = box(ctx, kBoxQualStatus);
    if (st != ~0ull) {
        if (bad_read) *bad_read = (int64_t)(st >> 8);
        char buf[160];
        std::snprintf(buf, sizeof(buf), "quality line of read %lld: its length differs from the bases kept, or a "
                                        "byte lies outside '!'..'~'", (long long)(st >> 8));
        return set_err(ctx, (int)(st & 0xFF), buf);
    }
    ctx->qual.blocks = (n_reads + block_reads - 1) / block_reads;
    ctx->qual.words = box(ctx, kBoxQualWords);
    ctx->qual.smoothed = box(ctx, kBoxQualSmoothed);
    ctx->qual.smoothed_total += ctx->qual.smoothed;
    ctx->qual.reads = n_reads;
    ctx->qual.block_reads = block_reads;
    return NTC_OK;
}
int q_unsupported(ntc_ctx *ctx, const char *call) {
    return set_err(ctx, NTC_ERR_UNSUPPORTED, std::string(call) + " takes bases without quality lines: qualities keep / "
                                             "bin8 need ntc_encode_pack_fastq");
}

// Decode side, coder 1 (ntc_decode_set_qualities checked every body with qr_body_ok): the
// blocks, where every span's stream starts and ends, and the payload go up; then as q_unpack.
int q_rans_decode(ntc_ctx *ctx, const std::vector<ntc_qual_meta> &metas, const std::vector<uint64_t> &payload,
                  uint64_t n_reads, uint64_t n_bases, const uint64_t *d_offs, uint8_t **d_quals) {
    const uint64_t nb = metas.size();
    std::vector<QRDecBlock> blk(nb + 1);
    std::vector<uint64_t> span_at;
    const uint8_t *pay = (const uint8_t *)payload.data();
    uint64_t r = 0;
    for (uint64_t b = 0; b < nb; b++) {
        const ntc_qual_meta &m = metas[b];
        QRDecBlock &k = blk[b];
        std::memset(&k, 0, sizeof(k));
        k.r0 = r;
        k.r1 = r += m.n_reads;
        k.n_quals = m.n_quals;
        k.body_off = m.payload_off;
        k.span_off = span_at.size() / 2;
        k.n_syms = m.n_syms;
        std::memcpy(k.alphabet, m.alphabet, 96);
        if (r > n_reads) break;
        if (m.n_syms <= 1) continue;
        const uint64_t ns = qr_spans(m.n_quals), tb = qr_table_bytes(m.n_syms);
        uint64_t at = m.payload_off + tb + 4 * ns;
        for (uint64_t j = 0; j < ns; j++) {
            uint32_t size;
            std::memcpy(&size, pay + m.payload_off + tb + 4 * j, 4);
            span_at.push_back(at);
            span_at.push_back(at += size);
        }
    }
    if (r != n_reads) return set_err(ctx, NTC_ERR_FORMAT, "the quality sections do not cover exactly the reads decoded");
    std::memset(&blk[nb], 0, sizeof(QRDecBlock));
    blk[nb].span_off = span_at.size() / 2;
    void *in, *quals;
    int rc;
    const uint64_t blk_bytes = (blk.size() * sizeof(QRDecBlock) + 63) & ~63ull, at_bytes = (span_at.size() * 8 + 63) & ~63ull;
    if ((rc = ensure(ctx, WS_QD_IN, blk_bytes + at_bytes + payload.size() * 8 + 64, &in))) return rc;
    if ((rc = ensure(ctx, WS_QD_QUALS, n_bases + 64, &quals))) return rc;
    HIP_TRY(ctx, hipMemcpy(in, blk.data(), blk.size() * sizeof(QRDecBlock), hipMemcpyHostToDevice));
    if (!span_at.empty())
        HIP_TRY(ctx, hipMemcpy((uint8_t *)in + blk_bytes, span_at.data(), span_at.size() * 8, hipMemcpyHostToDevice));
    if (!payload.empty())
        HIP_TRY(ctx, hipMemcpy((uint8_t *)in + blk_bytes + at_bytes, payload.data(), payload.size() * 8, hipMemcpyHostToDevice));
    QRDecArgs a{};
    a.blocks = (const QRDecBlock *)in;
    a.n_blocks = nb;
    a.n_spans = span_at.size() / 2;
    a.span_at = (const uint64_t *)((uint8_t *)in + blk_bytes);
    a.payload = (const uint8_t *)in + blk_bytes + at_bytes;
    a.offs = d_offs;
    a.n_reads = n_reads;
    a.quals = (uint8_t *)quals;
    a.status = ctx->d_status;
    launch_quality_rans_decode(a, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    *d_quals = (uint8_t *)quals;
    return rebox_decode(ctx);
}

// Decode side: the sections over the decoded reads' offsets -> quality bytes (WS_QD_QUALS);
// then the status mailbox again, as the unpack may have set the status.
int q_unpack(ntc_ctx *ctx, const std::vector<ntc_qual_meta> &metas, const std::vector<uint64_t> &payload,
             uint64_t n_reads, uint64_t n_bases, const uint64_t *d_offs, uint8_t **d_quals) {
    if (!metas.empty() && metas[0].reserved[0] == 1) return q_rans_decode(ctx, metas, payload, n_reads, n_bases, d_offs, d_quals);
    const uint64_t nb = metas.size();
    std::vector<uint8_t> up(nb * sizeof(QDecBlock));
    uint64_t r = 0, max_q = 0;
    for (uint64_t b = 0; b < nb; b++) {
        const ntc_qual_meta &m = metas[b];
        QDecBlock k{};
        k.r0 = r;
        k.r1 = r += m.n_reads;
        k.n_quals = m.n_quals;
        k.word_off = m.payload_off / 8;
        k.w = m.width;
        k.n_syms = m.n_syms;
        std::memcpy(k.alphabet, m.alphabet, 96);
        std::memcpy(up.data() + b * sizeof(QDecBlock), &k, sizeof(k));
        max_q = std::max(max_q, m.n_quals);
        if (r > n_reads) break;
    }
    if (r != n_reads) return set_err(ctx, NTC_ERR_FORMAT, "the quality sections do not cover exactly the reads decoded");
    void *in, *quals;
    int rc;
    const uint64_t blk_bytes = (up.size() + 63) & ~63ull;
    if ((rc = ensure(ctx, WS_QD_IN, blk_bytes + payload.size() * 8 + 64, &in))) return rc;
    if ((rc = ensure(ctx, WS_QD_QUALS, n_bases + 64, &quals))) return rc;
    if (!up.empty()) HIP_TRY(ctx, hipMemcpy(in, up.data(), up.size(), hipMemcpyHostToDevice));
    if (!payload.empty())
        HIP_TRY(ctx, hipMemcpy((uint8_t *)in + blk_bytes, payload.data(), payload.size() * 8, hipMemcpyHostToDevice));
    QDecArgs a{};
    a.blocks = (const QDecBlock *)in;
    a.n_blocks = nb;
    a.tiles = quality_unpack_tiles(max_q);
    a.payload = (const uint64_t *)((uint8_t *)in + blk_bytes);
    a.offs = d_offs;
    a.n_reads = n_reads;
    a.quals = (uint8_t *)quals;
    a.status = ctx->d_status;
    launch_quality_unpack(a, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    *d_quals = (uint8_t *)quals;
    return rebox_decode(ctx);
}

// ---- read names (names.hip) -------------------------------------------------------------
// After a GPU FASTQ parse, beside the quality pass: measure, offsets, emit.  Asynchronous,
// with a status word of its own; the status and the payload's size reach the host in mailbox
// words kBoxNameStatus and kBoxNameBytes at the encode call's own status sync (n_collect).
// Mode 0 returns before anything is launched.
int n_pack(ntc_ctx *ctx, uint64_t n_reads, uint32_t block_reads) {
    if (ctx->names.mode == 0 || n_reads == 0) return NTC_OK;
    const uint64_t nb = (n_reads + block_reads - 1) / block_reads;
    const FastqArgs &f = ctx->fq_last;
    void *cols, *blk, *pay;
    int rc;
    // start, len, mid (u32), the two scans (u64), pre and suf (u8)
    const uint64_t n1 = n_reads + 1;
    if ((rc = ensure(ctx, WS_N_COLS, n1 * (3 * 4 + 2 * 8) + 2 * n_reads + 64, &cols))) return rc;
    if ((rc = ensure(ctx, WS_N_BLOCKS, 64 + (nb + 1) * sizeof(NBlock), &blk))) return rc;
    if ((rc = ensure(ctx, WS_N_PAYLOAD, names_payload_max(f.n_raw, n_reads, nb), &pay))) return rc;
    NEncArgs a{};
    a.raw = f.raw;
    a.n_raw = f.n_raw;
    a.nl = f.nl;
    a.n_nl_p = f.tile_base + fastq_tiles(f.n_raw);
    a.n_reads = n_reads;
    a.n_blocks = nb;
    a.block_reads = block_reads;
    a.mode = (uint32_t)ctx->names.mode;
    a.len_off = (uint64_t *)cols;
    a.mid_off = a.len_off + n1;
    a.start = (uint32_t *)(a.mid_off + n1);
    a.len = a.start + n1;
    a.mid = a.len + n1;
    a.ps = (uint8_t *)(a.mid + n1);
    a.tmp = f.tmp;
    a.status = (unsigned long long *)blk;
    a.blocks = (NBlock *)((uint8_t *)blk + 64);
    a.payload = (uint8_t *)pay;
    a.box = ctx->h_box;
    ctx->h_box[kBoxNameStatus] = ~0ull;  // (the last call's kernels are done: every encode call ends synchronised)
    ctx->h_box[kBoxNameBytes] = 0;
    ctx->names.d_start = a.start;
    ctx->names.d_len = a.len;
    launch_names_pack(a, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    return NTC_OK;
}
// After the encode call's sync: the names pass's verdict.  A name too long fails the call.
int n_collect(ntc_ctx *ctx, uint64_t n_reads, uint32_t block_reads, int64_t *bad_read) {
    if (ctx->names.mode == 0 || n_reads == 0) return NTC_OK;
    const uint64_t st = box(ctx, kBoxNameStatus);
    if (st != ~0ull) {
        if (bad_read) *bad_read = (int64_t)(st >> 8);
        char buf[160];
        std::snprintf(buf, sizeof(buf), "name of read %lld: longer than %u bytes", (long long)(st >> 8), kNMax);
        return set_err(ctx, (int)(st & 0xFF), buf);
    }
    ctx->names.blocks = (n_reads + block_reads - 1) / block_reads;
    ctx->names.bytes = box(ctx, kBoxNameBytes);
    return NTC_OK;
}
int n_unsupported(ntc_ctx *ctx, const char *call) {
    return set_err(ctx, NTC_ERR_UNSUPPORTED, std::string(call) + " takes bases without header lines: names keep / id "
                                             "need ntc_encode_pack_fastq");
}

// Decode side: the sections -> the names of the decoded reads, read by read (WS_ND_NAMES) and
// where each starts (*d_name_off, n_reads + 1 words); then the status mailbox again.
int n_expand(ntc_ctx *ctx, const std::vector<ntc_name_meta> &metas, const std::vector<uint64_t> &payload,
             uint64_t n_reads, uint8_t **d_names, uint64_t **d_name_off) {
    const uint64_t nb = metas.size();
    std::vector<NDecBlock> up(nb);
    uint64_t r = 0, max_reads = 0, name_bytes = 0;
    for (uint64_t b = 0; b < nb; b++) {
        const ntc_name_meta &m = metas[b];
        up[b].r0 = r;
        up[b].r1 = r += m.n_reads;
        up[b].name_bytes = m.name_bytes;
        up[b].mid_bytes = m.mid_bytes;
        up[b].payload_off = m.payload_off;
        max_reads = std::max(max_reads, m.n_reads);
        name_bytes += m.name_bytes;
    }
    void *in, *cols, *names;
    int rc;
    const uint64_t blk_bytes = (nb * sizeof(NDecBlock) + 63) & ~63ull, n1 = n_reads + 1;
    if ((rc = ensure(ctx, WS_ND_IN, blk_bytes + payload.size() * 8 + 64, &in))) return rc;
    if ((rc = ensure(ctx, WS_ND_COLS, n1 * (2 * 8 + 2 * 4) + scan_tmp_words(n1) * 8 + 64, &cols))) return rc;
    if ((rc = ensure(ctx, WS_ND_NAMES, name_bytes + 64, &names))) return rc;
    if (nb) HIP_TRY(ctx, hipMemcpy(in, up.data(), nb * sizeof(NDecBlock), hipMemcpyHostToDevice));
    if (!payload.empty())
        HIP_TRY(ctx, hipMemcpy((uint8_t *)in + blk_bytes, payload.data(), payload.size() * 8, hipMemcpyHostToDevice));
    NDecArgs a{};
    a.blocks = (const NDecBlock *)in;
    a.n_blocks = nb;
    a.max_reads = max_reads;
    a.payload = (const uint8_t *)in + blk_bytes;
    a.payload_bytes = payload.size() * 8;
    a.n_reads = n_reads;
    a.name_off = (uint64_t *)cols;
    a.mid_off = a.name_off + n1;
    a.tmp = a.mid_off + n1;
    a.len = (uint32_t *)(a.tmp + scan_tmp_words(n1));
    a.mid = a.len + n1;
    a.names = (uint8_t *)names;
    a.names_cap = name_bytes;
    a.status = ctx->d_status;
    launch_names_expand(a, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    *d_names = (uint8_t *)names;
    *d_name_off = a.name_off;
    return rebox_decode(ctx);
}

// ---- content digests (digest.hip) ---------------------------------------------------------
// Encode side, option "digests" 1: a table entry per block (WS_DG_TABLE, the public
// ntc_digest_meta), each component added to it by one pass over bytes the call has in HBM
// anyway.  Asynchronous, on the call's stream; option 0 launches nothing.
static_assert(sizeof(DigestMetaDev) == sizeof(ntc_digest_meta) && sizeof(ntc_digest_meta) == 56,
              "the device table is the public meta");
// the components a call under the context's options yields (0: digests are off)
uint32_t dg_components(const ntc_ctx *ctx, bool fastq) {
    if (!ctx->dig.opt) return 0;
    return kDgSeq | (ctx->nx.policy == 2 ? kDgSym : 0) | (fastq && ctx->qual.mode ? kDgQual : 0) |
           (fastq && ctx->names.mode ? kDgName : 0);
}
// the table of the call: reads and bases per block, the digests zeroed but those in keep
int dg_init(ntc_ctx *ctx, const uint64_t *d_offs, uint64_t n_reads, uint32_t block_reads, uint32_t components,
            uint32_t keep) {
    const uint64_t nb = (n_reads + block_reads - 1) / block_reads;
    void *t;
    int rc;
    if ((rc = ensure(ctx, WS_DG_TABLE, nb * sizeof(DigestMetaDev), &t))) return rc;
    launch_digest_init((DigestMetaDev *)t, nb, n_reads, block_reads, d_offs, components, keep, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    return NTC_OK;
}
// component c (0 seq .. 3 name) of the call's blocks: strings by offs, or by start / len
int dg_add(ntc_ctx *ctx, uint32_t c, const void *buf, uint64_t buf_bytes, const uint64_t *offs, const uint32_t *start,
           const uint32_t *len, uint64_t n_reads, uint32_t block_reads) {
    DigestArgs a{};
    a.buf = (const uint8_t *)buf;
    a.buf_bytes = buf_bytes;
    a.offs = offs;
    a.start = start;
    a.len = len;
    a.n_reads = n_reads;
    a.block_reads = block_reads;
    a.out = ((DigestMetaDev *)ctx->ws[WS_DG_TABLE].p)->d + c;
    a.out_stride = sizeof(DigestMetaDev) / 8;
    launch_digest(a, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    return NTC_OK;
}

// The decode call in flight: expected and computed tables and the blocks' first reads on the
// device (WS_DGD_IN); the runs of sections of one size, each of which is one launch_digest
struct DgDecode {
    DigestMetaDev *expected = nullptr, *computed = nullptr;
    uint64_t *r0 = nullptr;
    std::vector<uint64_t> first;               // first read of each block, and the total
    std::vector<std::pair<uint64_t, uint64_t>> groups;  // [first block, one past the last)
    uint32_t checkable = kDgSeq;
};
int dgd_begin(ntc_ctx *ctx, const std::vector<ntc_digest_meta> &exp, DgDecode &d) {
    const uint64_t nb = exp.size();
    d.first.assign(nb + 1, 0);
    for (uint64_t b = 0; b < nb; b++) d.first[b + 1] = d.first[b] + exp[b].n_reads;
    for (uint64_t b = 0; b < nb;) {  // sections of exp[b].n_reads reads, closed by the first shorter one
        uint64_t e = b + 1;
        while (e < nb && exp[e - 1].n_reads == exp[b].n_reads && exp[e].n_reads <= exp[b].n_reads) e++;
        d.groups.emplace_back(b, e);
        b = e;
    }
    ctx->dig.expected = exp;
    ctx->dig.checkable = 0;
    ctx->dig.computed.assign(nb, ntc_digest_meta{});
    for (uint64_t b = 0; b < nb; b++) ctx->dig.computed[b].n_reads = exp[b].n_reads;
    void *in;
    int rc;
    const uint64_t tb = nb * sizeof(DigestMetaDev);
    if ((rc = ensure(ctx, WS_DGD_IN, 2 * tb + (nb + 1) * 8, &in))) return rc;
    d.expected = (DigestMetaDev *)in;
    d.computed = d.expected + nb;
    d.r0 = (uint64_t *)(d.computed + nb);
    HIP_TRY(ctx, hipMemcpy(d.expected, exp.data(), tb, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(d.computed, ctx->dig.computed.data(), tb, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(d.r0, d.first.data(), (nb + 1) * 8, hipMemcpyHostToDevice));
    return NTC_OK;
}
// component c of the decoded strings: buf by offs (n_reads + 1 words, positions relative to offs[0])
int dgd_add(ntc_ctx *ctx, DgDecode &d, uint32_t c, const void *buf, uint64_t buf_bytes, const uint64_t *offs) {
    d.checkable |= 1u << c;
    for (const auto &g : d.groups) {
        DigestArgs a{};
        a.buf = (const uint8_t *)buf;
        a.buf_bytes = buf_bytes;
        a.offs = offs + d.first[g.first];
        a.origin = offs;
        a.n_reads = d.first[g.second] - d.first[g.first];
        a.block_reads = (uint32_t)ctx->dig.expected[g.first].n_reads;
        a.out = d.computed[g.first].d + c;
        a.out_stride = sizeof(DigestMetaDev) / 8;
        a.status = ctx->d_status;
        launch_digest(a, ctx->stream);
    }
    HIP_TRY(ctx, hipGetLastError());
    return NTC_OK;
}
// the comparison on the device, the mailbox again (it may have set the status), and the
// computed table on its way to the host: it arrives with the call's own synchronisation
int dgd_compare(ntc_ctx *ctx, DgDecode &d, uint64_t n_reads, const uint64_t *d_offs) {
    DigestCmpArgs a{};
    a.expected = d.expected;
    a.computed = d.computed;
    a.r0 = d.r0;
    a.n_blocks = ctx->dig.expected.size();
    a.n_reads = n_reads;
    a.offs = d_offs;
    a.checkable = d.checkable;
    a.status = ctx->d_status;
    launch_digest_compare(a, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    if (const int rc = rebox_decode(ctx)) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->dig.computed.data(), d.computed, a.n_blocks * sizeof(DigestMetaDev),
                                hipMemcpyDeviceToHost, ctx->stream));
    ctx->dig.checkable = d.checkable;
    return NTC_OK;
}
// After the call's synchronisation: which components were checked, and for NTC_ERR_DIGEST the
// message: the lowest block that differs, the component, both values
int dgd_verdict(ntc_ctx *ctx, int rc) {
    static const char *const names[4] = {"seq", "sym", "qual", "name"};
    std::string msg;
    for (size_t b = 0; b < ctx->dig.expected.size(); b++) {
        ntc_digest_meta &e = ctx->dig.expected[b], &g = ctx->dig.computed[b];
        const uint32_t check = e.components & ctx->dig.checkable;
        g.components = check;
        g.reserved = 0;
        const uint64_t ed[4] = {e.d_seq, e.d_sym, e.d_qual, e.d_name}, gd[4] = {g.d_seq, g.d_sym, g.d_qual, g.d_name};
        if (rc != NTC_ERR_DIGEST || !msg.empty()) continue;
        char buf[200];
        if (g.n_bases != e.n_bases) {
            std::snprintf(buf, sizeof(buf), "digest mismatch in block %llu, component seq: %llu bases expected, %llu decoded",
                          (unsigned long long)b, (unsigned long long)e.n_bases, (unsigned long long)g.n_bases);
            msg = buf;
        }
        for (uint32_t c = 0; c < 4 && msg.empty(); c++)
            if ((check >> c & 1) && ed[c] != gd[c]) {
                std::snprintf(buf, sizeof(buf), "digest mismatch in block %llu, component %s: expected 0x%016llx, computed 0x%016llx",
                              (unsigned long long)b, names[c], (unsigned long long)ed[c], (unsigned long long)gd[c]);
                msg = buf;
            }
    }
    if (rc == NTC_ERR_DIGEST && !msg.empty()) ctx->err = msg;
    return rc;
}

// GPU packer (pack.hip) over the records of n_reads reads in HBM: block b = reads
// [b * block_reads, ...).  Pass 1 on the device, Rice parameters and payload layout on the
// host (glibc f64 math, codec_params.h), pass 2 on the device.  Synchronous.
int pack_blocks_impl(ntc_ctx *ctx, const uint64_t *d_recs, const uint64_t *d_roffs, uint64_t n_reads,
                     uint32_t block_reads, uint8_t *d_payload, uint64_t payload_capacity, ntc_block_meta *meta,
                     uint64_t *payload_bytes, const uint64_t *known_ends = nullptr) {
    *payload_bytes = 0;
    const uint64_t n_blocks = (n_reads + block_reads - 1) / block_reads;
    if (n_blocks == 0) return NTC_OK;
    for (int i = 0; i < 3; i++)
        if (!ctx->pack_ev[i]) HIP_TRY(ctx, hipEventCreate(&ctx->pack_ev[i]));
    uint64_t ends[2] = {0, 0};  // the record offsets' first and last values
    if (known_ends) {
        ends[0] = known_ends[0];
        ends[1] = known_ends[1];
    } else {
        HIP_TRY(ctx, hipMemcpyAsync(&ends[0], d_roffs, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(&ends[1], d_roffs + n_reads, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (ends[1] < ends[0]) return set_err(ctx, NTC_ERR_INVALID_ARG, "record offsets decrease");
    void *d_chunks, *d_meta;
    int rc;
    // chunks of block b at rec_begin + rec_begin / 31 + 2 b (pack.hip chunk_base: room for
    // 32 bases in every short record)
    const uint64_t chunk_words = ends[1] + ends[1] / 31 + 2 * n_blocks + 2;
    if ((rc = ensure(ctx, WS_PACK_CHUNKS, chunk_words * 8, &d_chunks))) return rc;
    const uint64_t meta_bytes = n_blocks * (sizeof(PackStats) + sizeof(PackParams) + 32) +
                                pack_stats_scratch_words(n_blocks, block_reads) * 8;
    if ((rc = ensure(ctx, WS_PACK_META, meta_bytes, &d_meta))) return rc;
    PackStats *d_stats = (PackStats *)d_meta;
    PackParams *d_params = (PackParams *)(d_stats + n_blocks);
    uint64_t *d_bits = (uint64_t *)(d_params + n_blocks);
    HIP_TRY(ctx, hipEventRecord(ctx->pack_ev[0], ctx->stream));
    launch_pack_stats(d_recs, d_roffs, n_reads, block_reads, n_blocks, (uint64_t *)d_chunks, chunk_words,
                      d_bits + 4 * n_blocks, d_stats, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ctx->pack_ev[1], ctx->stream));
    std::vector<PackStats> st(n_blocks);
    std::vector<PackParams> pp(n_blocks);
    HIP_TRY(ctx, hipMemcpyAsync(st.data(), d_stats, n_blocks * sizeof(PackStats), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    float ms1 = 0;
    HIP_TRY(ctx, hipEventElapsedTime(&ms1, ctx->pack_ev[0], ctx->pack_ev[1]));
    uint64_t words = 0;  // payload words so far (each stream at its exact upper bound)
    for (uint64_t b = 0; b < n_blocks; b++) {
        const PackStats &S = st[b];
        PackParams &P = pp[b];
        ntc_block_meta &M = meta[b];
        std::memset(&M, 0, sizeof(M));
        std::memset(&P, 0, sizeof(P));
        const uint64_t r0 = b * block_reads;
        M.num_records = std::min<uint64_t>(block_reads, n_reads - r0);
        M.n_recs = S.n_recs;
        M.status = NTC_OK;
        if (S.bad) M.status = NTC_ERR_FORMAT;  // a short record past 32 bases (from_2bit panics)
        else if (S.n_recs == 0 || S.n_long == 0 || S.T == 0) M.status = NTC_ERR_EMPTY_READ;  // App. B.3
        if (M.status != NTC_OK) {
            P.skip = 1;
            continue;
        }
        const uint64_t m1 = S.max1 + 2, m4 = S.max4 + 2;
        P.l1 = 63 - __builtin_clzll(m1);
        P.l4 = 63 - __builtin_clzll(m4);
        P.lim1 = (2ULL << P.l1) - m1;
        P.lim4 = (2ULL << P.l4) - m4;  // l4 <= 62
        P.p2 = ntc_rice_log2_b(S.n_long, S.sum2);
        P.p3 = ntc_rice_log2_b(S.n_recs, S.sum3);
        const uint64_t nch = (S.T + 30) / 31;
        const uint64_t bound[4] = {S.n_long * (uint64_t)(P.l1 + 1),
                                   S.n_long * (uint64_t)(1 + P.p2) + (S.sum2 >> P.p2),
                                   S.n_recs * (uint64_t)(1 + P.p3) + (S.sum3 >> P.p3),
                                   nch * (uint64_t)(P.l4 + 1)};
        const uint64_t params[4] = {m1, (uint64_t)P.p2, (uint64_t)P.p3, m4};
        const uint64_t counts[4] = {S.n_long, S.n_long, S.n_recs, nch};
        for (int k = 0; k < 4; k++) {
            P.off[k] = words;
            M.stream[k].offset = words * 8;
            M.stream[k].encoded_size = (bound[k] + 63) / 64;  // refined after pass 2
            M.stream[k].param = params[k];
            M.stream[k].num_u64 = counts[k];
            words += (bound[k] + 63) / 64 + 1;
        }
    }
    *payload_bytes = words * 8;
    if (words * 8 > payload_capacity) return set_err(ctx, NTC_ERR_CAPACITY, "payload_capacity too small");
    // pass 2 in segments (pack.hip k_pack_write): each block's records, then its s4 chunks
    std::vector<PackSeg> segs;
    for (uint64_t b = 0; b < n_blocks; b++) {
        PackParams &P = pp[b];
        P.seg0 = (uint32_t)segs.size();
        if (!P.skip) {
            const PackStats &S = st[b];
            for (uint64_t f = S.rec_begin; f < S.rec_begin + S.n_recs; f += kPackSegRecs)
                segs.push_back(PackSeg{(uint32_t)b, 0u, f, std::min<uint64_t>(kPackSegRecs, S.rec_begin + S.n_recs - f)});
            const uint64_t nch = (S.T + 30) / 31;
            for (uint64_t f = 0; f < nch; f += kPackSegChunks)
                segs.push_back(PackSeg{(uint32_t)b, 1u, f, std::min<uint64_t>(kPackSegChunks, nch - f)});
        }
        P.nseg = (uint32_t)segs.size() - P.seg0;
    }
    void *d_segs;
    if ((rc = ensure(ctx, WS_PACK_SEGS, segs.size() * (sizeof(PackSeg) + 48) + 64, &d_segs))) return rc;
    uint64_t *d_seg_bits = (uint64_t *)((uint8_t *)d_segs + segs.size() * sizeof(PackSeg));
    uint64_t *d_seg_start = d_seg_bits + 3 * segs.size();
    HIP_TRY(ctx, hipMemsetAsync(d_payload, 0, words * 8, ctx->stream));  // shared words and fallback tiles OR into zeros
    HIP_TRY(ctx, hipMemcpyAsync(d_params, pp.data(), n_blocks * sizeof(PackParams), hipMemcpyHostToDevice,
                                ctx->stream));
    if (!segs.empty())
        HIP_TRY(ctx, hipMemcpyAsync(d_segs, segs.data(), segs.size() * sizeof(PackSeg), hipMemcpyHostToDevice,
                                    ctx->stream));
    HIP_TRY(ctx, hipEventRecord(ctx->pack_ev[2], ctx->stream));
    launch_pack_write(d_recs, (const uint64_t *)d_chunks, d_stats, d_params, n_blocks, (const PackSeg *)d_segs,
                      segs.size(), d_seg_bits, d_seg_start, (uint64_t *)d_payload, d_bits, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ctx->pack_ev[1], ctx->stream));
    std::vector<uint64_t> bits(n_blocks * 4);
    HIP_TRY(ctx, hipMemcpyAsync(bits.data(), d_bits, n_blocks * 32, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    float ms2 = 0;
    HIP_TRY(ctx, hipEventElapsedTime(&ms2, ctx->pack_ev[2], ctx->pack_ev[1]));
    ctx->last_pack_ms = (double)ms1 + (double)ms2;
    for (uint64_t b = 0; b < n_blocks; b++) {
        if (meta[b].status != NTC_OK) continue;
        for (int k = 0; k < 4; k++) {
            const uint64_t w = (bits[b * 4 + k] + 63) / 64;
            if (w > meta[b].stream[k].encoded_size)
                return set_err(ctx, NTC_ERR_FORMAT, "packer exceeded its stream bound");  // never expected
            meta[b].stream[k].encoded_size = w;
        }
    }
    return NTC_OK;
}

}  // namespace

extern "C" {

int ntc_abi_version(void) { return NTC_ABI_VERSION; }

int ntc_ctx_create(int device, ntc_ctx **out) {
    if (!out) return NTC_ERR_INVALID_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return NTC_ERR_HIP;
    if (device < 0 || device >= ndev) return NTC_ERR_INVALID_ARG;
    ntc_ctx *ctx = new ntc_ctx();
    ctx->device = device;
    // how a host thread waits for the device (A/B hook; HIP's default is auto): "spin",
    // "yield" or "blocking".  Takes effect only before the device's first use in the process.
    if (const char *v = std::getenv("NTC_DEVICE_SCHEDULE")) {
        const unsigned f = std::strcmp(v, "spin") == 0       ? hipDeviceScheduleSpin
                           : std::strcmp(v, "yield") == 0    ? hipDeviceScheduleYield
                           : std::strcmp(v, "blocking") == 0 ? hipDeviceScheduleBlockingSync
                                                             : hipDeviceScheduleAuto;
        if (hipSetDevice(device) == hipSuccess && hipSetDeviceFlags(f) != hipSuccess) (void)hipGetLastError();
    }
    if (hipSetDevice(device) != hipSuccess ||
        hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess ||
        hipMalloc((void **)&ctx->d_status, 64) != hipSuccess ||
        hipHostMalloc((void **)&ctx->h_box, kBoxWords * 8, hipHostMallocDefault) != hipSuccess) {
        delete ctx;
        return NTC_ERR_HIP;
    }
    for (auto &e : ctx->ev)
        if (hipEventCreate(&e) != hipSuccess) {
            delete ctx;
            return NTC_ERR_HIP;
        }
    if (hipDeviceGetAttribute(&ctx->num_cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess ||
        ctx->num_cus <= 0)
        ctx->num_cus = 256;
    if (const char *v = std::getenv("NTC_ENCODE_VARIANT")) {
        int x = std::atoi(v);
        if (x == 1 || x == 4) ctx->encode_variant = x;
    }
    *out = ctx;
    return NTC_OK;
}

void ntc_ctx_destroy(ntc_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    for (auto &b : ctx->ws)
        if (b.p) (void)hipFree(b.p);
    ctx->index_mem.reset();
    if (ctx->d_status) (void)hipFree(ctx->d_status);
    if (ctx->h_box) (void)hipHostFree(ctx->h_box);
    for (auto &e : ctx->ev)
        if (e) (void)hipEventDestroy(e);
    for (auto &e : ctx->pack_ev)
        if (e) (void)hipEventDestroy(e);
    if (ctx->stream && ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

const char *ntc_last_error(const ntc_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int ntc_ctx_set_stream(ntc_ctx *ctx, void *hip_stream) {
    if (!ctx) return NTC_ERR_INVALID_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->own_stream) HIP_TRY(ctx, hipStreamDestroy(ctx->stream));
    if (hip_stream) {
        ctx->stream = (hipStream_t)hip_stream;
        ctx->own_stream = false;
    } else {
        HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
        ctx->own_stream = true;
    }
    return NTC_OK;
}

int ntc_ctx_synchronize(ntc_ctx *ctx) {
    if (!ctx) return NTC_ERR_INVALID_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return NTC_OK;
}

int ntc_index_share(ntc_ctx *dst, const ntc_ctx *src) {
    if (!dst || !src) return set_err(dst, NTC_ERR_INVALID_ARG, "null context");
    if (!src->has_index) return set_err(dst, NTC_ERR_NO_INDEX, "the source context holds no index");
    if (src->device != dst->device) return set_err(dst, NTC_ERR_INVALID_ARG, "contexts on different devices");
    if (dst == src) return NTC_OK;
    HIP_TRY(dst, hipSetDevice(dst->device));
    HIP_TRY(dst, hipStreamSynchronize(dst->stream));
    dst->index_mem = src->index_mem;
    dst->dix = src->dix;
    dst->index_bytes = src->index_bytes;
    dst->n_paths = src->n_paths;
    dst->path_text_len = src->path_text_len;
    dst->filter_density_ppm = src->filter_density_ppm;
    dst->tab_u_fallback = src->tab_u_fallback;
    dst->index_decode_only = src->index_decode_only;
    dst->upload_host_us = dst->upload_total_us = 0;
    dst->has_index = true;
    return NTC_OK;
}

}  // extern "C"

// the host half of an upload: the index copied out of the view and its derived tables
// (derived.cpp build_derived), no GPU involved
struct ntc_index_prep {
    HostIndex hx;
    Derived dv;
    int64_t host_us = 0;
};

namespace {
int prepare_index(const ntc_index_view *v, ntc_index_prep &p, std::string &err) {
    const auto t0 = std::chrono::steady_clock::now();
    p.hx.n = v->n_nodes;
    p.hx.k = v->k;
    const uint64_t nw = (v->n_nodes + 63) / 64;
    for (int c = 0; c < 4; c++) {
        p.hx.rows[c].assign(v->rows[c], v->rows[c] + nw);
        p.hx.C[c] = v->C[c];
    }
    p.hx.lcs.assign(v->lcs, v->lcs + v->n_nodes);
    if (!build_derived(p.hx, p.dv, err, false)) return NTC_ERR_FORMAT;
    p.host_us = (int64_t)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0)
                    .count();
    return NTC_OK;
}
bool view_ok(const ntc_index_view *v) {
    if (!v || !v->lcs) return false;
    for (int c = 0; c < 4; c++)
        if (!v->rows[c]) return false;
    return true;
}
int upload_prepared(ntc_ctx *ctx, const ntc_index_prep &prep);
}  // namespace

extern "C" {

int ntc_index_prepare(const ntc_index_view *v, ntc_index_prep **out) {
    if (!out || !view_ok(v)) return NTC_ERR_INVALID_ARG;
    *out = nullptr;
    auto *p = new (std::nothrow) ntc_index_prep();
    if (!p) return NTC_ERR_CAPACITY;
    std::string err;
    const int rc = prepare_index(v, *p, err);
    if (rc) {
        delete p;
        return rc;
    }
    *out = p;
    return NTC_OK;
}

void ntc_index_prep_free(ntc_index_prep *p) { delete p; }

int ntc_index_upload_prepared(ntc_ctx *ctx, const ntc_index_prep *p) {
    if (!ctx || !p) return set_err(ctx, NTC_ERR_INVALID_ARG, "null context or prepared index");
    return upload_prepared(ctx, *p);
}

int ntc_index_upload(ntc_ctx *ctx, const ntc_index_view *v) {
    if (!ctx || !view_ok(v)) return set_err(ctx, NTC_ERR_INVALID_ARG, "null index view");
    ntc_index_prep p;
    std::string err;
    const int rc = prepare_index(v, p, err);
    if (rc) return set_err(ctx, rc, err);
    return upload_prepared(ctx, p);
}

}  // extern "C"

namespace {
// ---- the device half of an upload -----------------------------------------------------------
// One upload in flight: what its stages (up_*, below in the order they run) hand to one another.
struct Upload {
    ntc_ctx *ctx;
    const HostIndex &hx;
    const Derived &dv;
    const uint64_t n;  // nodes
    const int64_t host_us;
    const std::chrono::steady_clock::time_point t_start = std::chrono::steady_clock::now();
    // the raw arrays of the index, and the walk build's inputs and buffers (freed after the path cover)
    void *d_lines = nullptr, *d_lcs = nullptr, *d_uniq = nullptr, *d_walk = nullptr;
    void *d_walk_a = nullptr, *d_walk_b = nullptr, *d_pred = nullptr, *d_code = nullptr;
    // the path cover: has_paths says that it was built and fits 31 bits
    void *d_pstream = nullptr, *d_colex_at = nullptr, *d_pos = nullptr, *d_puniq = nullptr;
    bool has_paths = false, uniq_hint = false;
    uint64_t tlen = 0, n_paths = 0;
    // the suffix table: levels 1..U, its presence bits, those of the filter level (F != 0)
    uint32_t U = 0;
    void *d_tab = nullptr, *d_bits = nullptr, *d_fbits = nullptr;

    Upload(ntc_ctx *c, const ntc_index_prep &p) : ctx(c), hx(p.hx), dv(p.dv), n(p.hx.n), host_us(p.host_us) {}
    // memory of the index itself: freed with the last context that holds it
    int dalloc(uint64_t bytes, void **p) {
        HIP_TRY(ctx, hipMalloc(p, bytes));
        ctx->index_mem->ptrs.push_back(*p);
        ctx->index_bytes += bytes;
        return NTC_OK;
    }
    double seconds() const { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count(); }
    // NTC_UPLOAD_TRACE=1: seconds since the start of the device half at each stage (stderr)
    void mark(const char *what, bool sync) const {
        static const bool trace = std::getenv("NTC_UPLOAD_TRACE") != nullptr;
        if (!trace) return;
        if (sync) (void)hipStreamSynchronize(ctx->stream);
        std::fprintf(stderr, "[upload] %-28s %.4f s\n", what, seconds());
    }
};

int up_free_previous(Upload &u) {
    ntc_ctx *ctx = u.ctx;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->index_mem = std::make_shared<IndexMem>(ctx->device);  // the previous one goes with its last holder
    ctx->has_index = false;
    ctx->index_bytes = 0;
    return NTC_OK;
}

int up_raw_arrays(Upload &u) {
    ntc_ctx *ctx = u.ctx;
    const uint64_t n = u.n;
    int rc;
    if ((rc = u.dalloc(u.dv.rank.size() * sizeof(uint2), &u.d_lines))) return rc;
    if ((rc = u.dalloc(n + 256, &u.d_lcs))) return rc;
    if ((rc = u.dalloc(u.dv.uniq.size() * 4, &u.d_uniq))) return rc;
    if ((rc = u.dalloc(n * sizeof(WalkEntry), &u.d_walk))) return rc;
    HIP_TRY(ctx, hipMalloc(&u.d_walk_a, n * sizeof(WalkStep)));
    HIP_TRY(ctx, hipMalloc(&u.d_walk_b, n * sizeof(WalkStep)));
    HIP_TRY(ctx, hipMalloc(&u.d_pred, n * 4));
    HIP_TRY(ctx, hipMalloc(&u.d_code, n + 64));
    HIP_TRY(ctx, hipMemcpy(u.d_lines, u.dv.rank.data(), u.dv.rank.size() * sizeof(uint2), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemset(u.d_lcs, 0, n + 256));
    HIP_TRY(ctx, hipMemcpy(u.d_lcs, u.hx.lcs.data(), n, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(u.d_uniq, u.dv.uniq.data(), u.dv.uniq.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(u.d_pred, u.dv.pred.data(), n * 4, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(u.d_code, u.dv.code.data(), n, hipMemcpyHostToDevice));
    u.mark("allocations + H2D", false);
    return NTC_OK;
}

int up_walk_table(Upload &u) {
    launch_walk_build((const uint32_t *)u.d_pred, (const uint8_t *)u.d_code, u.n, (WalkStep *)u.d_walk_a,
                      (WalkStep *)u.d_walk_b, (WalkEntry *)u.d_walk, u.ctx->stream);
    HIP_TRY(u.ctx, hipGetLastError());
    u.mark("walk table", true);
    return NTC_OK;
}

// path cover, built on the device (kernels.hip "path cover"; derived.cpp build_paths is the
// same cover on the host, for emulation); a decode-only upload has none
int up_path_cover(Upload &u, bool dec_only) {
    ntc_ctx *ctx = u.ctx;
    const HostIndex &hx = u.hx;
    const Derived &dv = u.dv;
    const uint64_t n = u.n;
    int rc;
    ctx->index_decode_only = false;
    if (!dec_only && n < (1ULL << 31)) {
        const std::vector<uint8_t> dummy = dummy_nodes(hx, dv);
        std::vector<uint32_t> dbits(n / 32 + 2, 0);
        for (uint64_t z = 0; z < n; z++)
            if (dummy[z]) dbits[z >> 5] |= 1u << (z & 31);
        std::vector<void *> tmp;
        auto talloc = [&](uint64_t bytes, void **p) -> int {
            HIP_TRY(ctx, hipMalloc(p, bytes));
            tmp.push_back(*p);
            return NTC_OK;
        };
        auto free_tmp = [&]() {
            (void)hipStreamSynchronize(ctx->stream);
            for (void *p : tmp) (void)hipFree(p);
            tmp.clear();
        };
        void *d_dummy, *d_prv, *d_sta, *d_stb, *d_len, *d_vals, *d_base, *d_stmp, *d_cnt;
        if ((rc = talloc(dbits.size() * 4, &d_dummy)) || (rc = talloc(n * 4, &d_prv)) ||
            (rc = talloc(n * 16, &d_sta)) || (rc = talloc(n * 16, &d_stb)) || (rc = talloc(n * 4, &d_len)) ||
            (rc = talloc(n * 4, &d_vals)) || (rc = talloc((n + 1) * 8, &d_base)) ||
            (rc = talloc(scan_tmp_words(n) * 8, &d_stmp)) || (rc = talloc(16, &d_cnt))) {
            free_tmp();
            return rc;
        }
        HIP_TRY(ctx, hipMemcpy(d_dummy, dbits.data(), dbits.size() * 4, hipMemcpyHostToDevice));
        PathArgs pa{(const uint2 *)u.d_lines, dv.rwords, (uint32_t)n, hx.k, (const uint8_t *)u.d_lcs,
                    (const uint32_t *)d_dummy, (const uint32_t *)u.d_pred, (const uint8_t *)u.d_code,
                    (const uint32_t *)u.d_uniq};
        uint32_t *prv = (uint32_t *)d_prv, *cnt = (uint32_t *)d_cnt;
        HIP_TRY(ctx, hipMemsetAsync(prv, 0xFF, n * 4, ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(cnt, 0, 16, ctx->stream));
        launch_path_edges(pa, prv, ctx->stream);
        if (ctx->path_link_opt) {  // unitigs linked across branches (derived.cpp link_unitigs)
            void *d_want, *d_bpred;
            if ((rc = talloc(n * 4, &d_want)) || (rc = talloc(n * 8, &d_bpred))) {
                free_tmp();
                return rc;
            }
            const uint4 *su = launch_path_rank(prv, (uint32_t)n, (uint4 *)d_sta, (uint4 *)d_stb, ctx->stream);
            HIP_TRY(ctx, hipMemsetAsync(d_len, 0, n * 4, ctx->stream));
            launch_path_lengths(pa, su, prv, (uint32_t *)d_len, (uint32_t *)d_vals, cnt + 2, ctx->stream);
            HIP_TRY(ctx, hipMemsetAsync(d_want, 0xFF, n * 4, ctx->stream));
            HIP_TRY(ctx, hipMemsetAsync(d_bpred, 0xFF, n * 8, ctx->stream));
            launch_path_link(pa, su, (const uint32_t *)d_len, (uint32_t *)d_want, (unsigned long long *)d_bpred, prv,
                             ctx->stream);
        }
        const uint4 *st = launch_path_rank(prv, (uint32_t)n, (uint4 *)d_sta, (uint4 *)d_stb, ctx->stream);
        launch_path_cut(pa, st, prv, cnt, ctx->stream);
        uint32_t cut = 0;
        HIP_TRY(ctx, hipMemcpyAsync(&cut, cnt, 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (cut) st = launch_path_rank(prv, (uint32_t)n, (uint4 *)d_sta, (uint4 *)d_stb, ctx->stream);
        HIP_TRY(ctx, hipMemsetAsync(d_len, 0, n * 4, ctx->stream));
        launch_path_lengths(pa, st, prv, (uint32_t *)d_len, (uint32_t *)d_vals, cnt + 1, ctx->stream);
        scan_excl_u32((const uint32_t *)d_vals, n, (uint64_t *)d_base, (uint64_t *)d_stmp, ctx->stream);
        uint32_t np32 = 0;
        HIP_TRY(ctx, hipMemcpyAsync(&u.tlen, (uint64_t *)d_base + n, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(&np32, cnt + 1, 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        HIP_TRY(ctx, hipGetLastError());
        u.n_paths = np32;
        const uint64_t tlen = u.tlen;
        if (tlen + 64 < (1ULL << 31)) {
            // sizes as derived.cpp build_paths: groups read up to k + 64 characters past a node
            const uint64_t n_groups = (tlen + hx.k) / 32 + 8, n_colex = tlen + 8, n_puniq = tlen / 64 + 4;
            if ((rc = u.dalloc(n_puniq * 8, &u.d_puniq)) || (rc = u.dalloc(n_groups * 16, &u.d_pstream)) ||
                (rc = u.dalloc(n_colex * 4 + 64, &u.d_colex_at)) || (rc = u.dalloc(n * 4, &u.d_pos))) {
                free_tmp();
                return rc;
            }
            HIP_TRY(ctx, hipMemsetAsync(u.d_puniq, 0, n_puniq * 8, ctx->stream));
            HIP_TRY(ctx, hipMemsetAsync(u.d_pstream, 0, n_groups * 16, ctx->stream));
            HIP_TRY(ctx, hipMemsetAsync(u.d_colex_at, 0xFF, n_colex * 4 + 64, ctx->stream));
            HIP_TRY(ctx, hipMemsetAsync(u.d_pos, 0xFF, n * 4, ctx->stream));
            launch_path_place(pa, st, prv, (const uint64_t *)d_base, (uint32_t *)u.d_colex_at, (uint32_t *)u.d_pos,
                              (uint4 *)u.d_pstream, (uint64_t *)u.d_puniq, ctx->stream);
            if (hx.k >= kForkBlockMinK)
                launch_path_forks(pa, st, (const uint32_t *)d_len, (const uint64_t *)d_base, (const uint32_t *)u.d_pos,
                                  (const uint4 *)u.d_pstream, (uint32_t *)u.d_colex_at, ctx->stream);
            if (ctx->uniq_hint_opt != 0 && n <= kUniqHintMaxN) {
                launch_path_hint(hx.k, tlen, (const uint4 *)u.d_pstream, (const uint64_t *)u.d_puniq,
                                 (uint32_t *)u.d_colex_at, ctx->stream);
                u.uniq_hint = true;
            }
            HIP_TRY(ctx, hipGetLastError());
            u.has_paths = true;
        }
        free_tmp();
    }
    u.mark("path cover", true);
    // the walk build's inputs served the cover too: both are done with them
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipFree(u.d_walk_a));
    HIP_TRY(ctx, hipFree(u.d_walk_b));
    HIP_TRY(ctx, hipFree(u.d_pred));
    HIP_TRY(ctx, hipFree(u.d_code));
    return NTC_OK;
}

// the context's DevIndex so far, and the choice between the two k_ms4 builds
int up_joint_choice(Upload &u) {
    ntc_ctx *ctx = u.ctx;
    const bool has_paths = u.has_paths;
    DevIndex &d = ctx->dix;
    d = DevIndex{};  // (what the stages after this one do not build stays null / 0)
    d.rank = (const uint2 *)u.d_lines;
    d.lcs = (const uint8_t *)u.d_lcs;
    d.uniq = (const uint32_t *)u.d_uniq;
    d.walk = (const WalkEntry *)u.d_walk;
    d.rwords = u.dv.rwords;
    d.n = (uint32_t)u.n;
    d.k = u.hx.k;
    d.t_jump = u.dv.t_jump;
    for (int c = 0; c < 5; c++) d.C[c] = u.dv.C[c];
    d.has_paths = has_paths ? 1u : 0u;
    d.path_len = has_paths ? (uint32_t)u.tlen : 0u;
    d.pstream = (const uint4 *)u.d_pstream;
    d.colex_at = (const uint32_t *)u.d_colex_at;
    d.pos_of_node = (const uint32_t *)u.d_pos;
    d.puniq = (const uint64_t *)u.d_puniq;
    d.forks = has_paths && u.hx.k >= kForkBlockMinK ? 1u : 0u;
    d.uniq_hint = has_paths && u.uniq_hint ? 1u : 0u;
    d.node_mask = d.uniq_hint ? kNodeMaskHint : kNodeMaskPlain;
    d.absent = u.dv.absent;
    // Joint path runs pay off when MS intervals above U hold several nodes for long stretches:
    // genome collections, whose shared regions split the path cover into short unitigs (S91:
    // 1.19 M paths over 70 M nodes).  A cover of long paths (one genome, C91: 2 paths) keeps
    // the lighter k_ms4 build.
    d.joint = has_paths && (ctx->joint_opt == 1 || (ctx->joint_opt < 0 && u.n_paths * kJointAutoNodesPerPath > u.n))
                  ? 1u : 0u;
    return NTC_OK;
}

// suffix table, levels 1..U, built on the device from the rank lines (and before it, under the
// A/B option ext2, the two-character rank lines: 8 B per node)
int up_suffix_table(Upload &u) {
    ntc_ctx *ctx = u.ctx;
    DevIndex &d = ctx->dix;
    const uint64_t n = u.n;
    int rc;
    if (ctx->ext2_opt) {
        void *d_r2;
        if ((rc = u.dalloc(rank2_blocks(n) * 4 * sizeof(Rank2Chunk), &d_r2))) return rc;
        launch_rank2(d, (Rank2Chunk *)d_r2, ctx->stream);
        d.rank2 = (const Rank2Chunk *)d_r2;
    }
    uint32_t U = ctx->tab_u_opt ? std::min<uint32_t>(ctx->tab_u_opt, std::min<uint32_t>(u.hx.k, kTabMaxU))
                                : default_tab_u(n, u.hx.k, u.hx.lcs.data());
    ctx->tab_u_fallback = 0;
    if (!ctx->tab_u_opt && U > 14) {
        // the density rule's deeper table (U = 15: 11.5 GB against 2.9 GB) only where it fits
        // beside what the device already holds plus an encode workspace (ranks may share a GPU)
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess &&
            (uint64_t)free_b < tab_base(U + 1) * sizeof(uint2) + (64ull << 30)) {
            U = 14;
            ctx->tab_u_fallback = 1;
        }
    }
    if (hipMalloc(&u.d_tab, tab_base(U + 1) * sizeof(uint2)) != hipSuccess) {
        (void)hipGetLastError();
        if (ctx->tab_u_opt || U <= 14) return set_err(ctx, NTC_ERR_HIP, "suffix table allocation failed");
        U = 14;  // allocation failed at the deeper level: fall back (results never depend on U)
        ctx->tab_u_fallback = 1;
        if ((rc = u.dalloc(tab_base(U + 1) * sizeof(uint2), &u.d_tab))) return rc;
    } else {
        ctx->index_mem->ptrs.push_back(u.d_tab);
        ctx->index_bytes += tab_base(U + 1) * sizeof(uint2);
    }
    const uint32_t F = filter_level(U);
    if ((rc = u.dalloc(tab_bits_words(U) * 4, &u.d_bits))) return rc;
    if (F && (rc = u.dalloc(tab_bits_words(F) * 4, &u.d_fbits))) return rc;
    d.tab = (const uint2 *)u.d_tab;
    d.tab_bits = (const uint32_t *)u.d_bits;
    d.filt_bits = (const uint32_t *)u.d_fbits;
    d.filt_f = F;
    d.tab_u = u.U = U;
    d.tab_pos = (u.has_paths && U >= u.dv.t_jump && n < (1ULL << 31)) ? 1u : 0u;
    u.mark("suffix table allocation", false);
    launch_tab_build(d, U, (uint2 *)u.d_tab, (uint32_t *)u.d_bits, F, (uint32_t *)u.d_fbits, ctx->stream);
    u.mark("suffix table", true);
    return NTC_OK;
}

// what a SCAN reads: window words, the pre-filter's verdict, pair words
int up_scan_words(Upload &u) {
    ntc_ctx *ctx = u.ctx;
    DevIndex &d = ctx->dix;
    const uint32_t U = u.U, F = d.filt_f;
    int rc;
    // SCAN window words (a (U-3)-mer keyed 32-byte entry answers four positions): two lines
    // answer the eight positions of a SCAN unit.  k_ms4 is bound by its lane loads in the
    // CU's vector memory path (TA/TD 93-96 % busy at C91, TCP stalled on pending L2 data), and
    // the L2-resident filter took 18 of them per SCAN: C91 k_ms4 3.70 -> 2.40 ms with window
    // words and no filter.  Auto: on for every U >= 4, both builds.
    const bool win_on = U >= 4 && ctx->win_opt != 0;
    if (win_on) {
        void *d_win;
        if ((rc = u.dalloc(win_words_count(U) * 32, &d_win))) return rc;
        launch_win_words((const uint32_t *)u.d_bits, U, (uint32_t *)d_win, ctx->stream);
        d.win_w = (const uint32_t *)d_win;
    }
    ctx->filter_density_ppm = -1;
    if (F) {
        // A filter over a large index is mostly ones (S91's 70 M nodes: 72 % of all 12-mers)
        // and passes most positions, so it costs more lines than it saves: auto mode drops it
        // above kFiltMaxDensityPpm (every SCAN then goes straight to the exact pair words).
        std::vector<uint32_t> fb(tab_bits_words(F));
        HIP_TRY(ctx, hipMemcpyAsync(fb.data(), u.d_fbits, fb.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        uint64_t ones = 0;
        for (uint32_t x : fb) ones += (uint64_t)__builtin_popcount(x);
        ctx->filter_density_ppm = (int64_t)(ones * 1000000 / ((uint64_t)fb.size() * 32));
        // (auto: off with window words, whose loads do not depend on it)
        const bool on = ctx->filter_opt == 1 ||
                        (ctx->filter_opt < 0 && !win_on && ctx->filter_density_ppm <= kFiltMaxDensityPpm);
        if (!on) d.filt_f = 0;
    }
    if (ctx->pair_bytes_opt) {
        void *d_pair;
        if ((rc = u.dalloc((pair_words_count(U) + 1) / 2 * 4, &d_pair))) return rc;
        launch_pair_words((const uint2 *)u.d_tab + tab_base(U), U, (uint16_t *)d_pair, ctx->stream);
        d.pair_w = (const uint16_t *)d_pair;
    }
    return NTC_OK;
}

// substitution words (encode_core.h subst_clean), the fourth word of each path-stream group:
// k_ms4 without joint runs skips the SCAN after a run break at a set bit
int up_subst_words(Upload &u) {
    ntc_ctx *ctx = u.ctx;
    const DevIndex &d = ctx->dix;
    ctx->subst_built = 0;
    if (u.has_paths) {
        u.mark("SCAN words", true);
        const bool on = ctx->subst_opt != 0 && !d.joint && d.tab_pos && u.U >= 4;
        launch_subst_words(d, (uint4 *)u.d_pstream, pstream_groups(u.tlen, u.hx.k), on, ctx->stream);
        ctx->subst_built = on ? 1 : 0;
        u.mark("substitution words", true);
    }
    return NTC_OK;
}

int up_finish(Upload &u, bool dec_only) {
    ntc_ctx *ctx = u.ctx;
    // (decode reads the walk table alone: no suffix table, SCAN words or rank chunks)
    if (dec_only) ctx->subst_built = 0;
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->n_paths = u.n_paths;  // (a decode-only upload built no cover: both are 0)
    ctx->path_text_len = u.tlen;
    ctx->index_decode_only = dec_only;
    ctx->has_index = true;
    u.mark(dec_only ? "done (decode only)" : "done", false);
    ctx->upload_total_us = u.host_us + (int64_t)(u.seconds() * 1e6);
    return NTC_OK;
}

int upload_prepared(ntc_ctx *ctx, const ntc_index_prep &prep) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Upload u(ctx, prep);
    ctx->upload_host_us = prep.host_us;
    const bool dec_only = ctx->decode_only_opt != 0;
    int rc;
    if ((rc = up_free_previous(u)) || (rc = up_raw_arrays(u)) || (rc = up_walk_table(u)) ||
        (rc = up_path_cover(u, dec_only)) || (rc = up_joint_choice(u)))
        return rc;
    if (!dec_only && ((rc = up_suffix_table(u)) || (rc = up_scan_words(u)) || (rc = up_subst_words(u)))) return rc;
    return up_finish(u, dec_only);
}
}  // namespace

// ---- context options ----------------------------------------------------------------------
// One table drives ntc_ctx_set_option and ntc_ctx_get_option.  A row with a setter accepts the
// values lo..hi that its rule allows and answers msg to any other; a row without one is
// read-only (to set_option it is an unknown option), one without a getter write-only.
namespace {
enum OptRule { kInRange, kEndsOnly, kMultipleOf4 };
struct Option {
    const char *key;
    int64_t lo, hi;
    OptRule rule;
    const char *msg;
    int (*set)(ntc_ctx *, int64_t);
    int (*get)(const ntc_ctx *, int64_t *);
};
constexpr int64_t kNoMax = INT64_MAX;

// an action: copies of `value` bytes each way, now
int warm_dma(ntc_ctx *ctx, int64_t value) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    void *h = nullptr, *d = nullptr;
    if (hipHostMalloc(&h, (size_t)value, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return set_err(ctx, NTC_ERR_HIP, "warm_dma: pinned allocation failed");
    }
    int rc = ensure(ctx, WS_STAGE_BASES, (uint64_t)value, &d);
    if (rc == NTC_OK) {
        if (hipMemcpyAsync(h, d, (size_t)value, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
            hipMemcpyAsync(d, h, (size_t)value, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
            hipStreamSynchronize(ctx->stream) != hipSuccess) {
            (void)hipGetLastError();
            rc = set_err(ctx, NTC_ERR_HIP, "warm_dma: copy failed");
        }
    }
    (void)hipHostFree(h);
    return rc;
}
// test hook: overflow pools per read (entries, records)
int set_pool_per_read(ntc_ctx *ctx, int64_t value) {
    ctx->epool_per_read = ctx->rpool_per_read = (double)value;
    ctx->epool_per_base = ctx->rpool_per_base = 0.0;
    return NTC_OK;
}
// test hook: derived.h subst_word_hash of the device words
int get_subst_hash(const ntc_ctx *ctx, int64_t *value) {
    if (!ctx->has_index || !ctx->dix.has_paths) return NTC_ERR_NO_INDEX;
    std::vector<uint4> ps(pstream_groups(ctx->path_text_len, ctx->dix.k));
    if (hipSetDevice(ctx->device) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess ||
        hipMemcpy(ps.data(), ctx->dix.pstream, ps.size() * 16, hipMemcpyDeviceToHost) != hipSuccess)
        return NTC_ERR_HIP;
    *value = (int64_t)subst_word_hash(ps.data(), ps.size());
    return NTC_OK;
}
// test hook: derived.h path_cover_hash of the device cover
int get_path_hash(const ntc_ctx *ctx, int64_t *value) {
    if (!ctx->has_index || !ctx->dix.has_paths) return NTC_ERR_NO_INDEX;
    const uint64_t n = ctx->dix.n, k = ctx->dix.k, tlen = ctx->path_text_len;
    std::vector<uint4> ps((tlen + k) / 32 + 8);
    std::vector<uint32_t> ca(tlen + 8), pn(n);
    std::vector<uint64_t> pu(tlen / 64 + 4);
    if (hipSetDevice(ctx->device) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess ||
        hipMemcpy(ps.data(), ctx->dix.pstream, ps.size() * 16, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(ca.data(), ctx->dix.colex_at, ca.size() * 4, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(pn.data(), ctx->dix.pos_of_node, pn.size() * 4, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(pu.data(), ctx->dix.puniq, pu.size() * 8, hipMemcpyDeviceToHost) != hipSuccess)
        return NTC_ERR_HIP;
    *value = (int64_t)path_cover_hash(ps.data(), ca.data(), pn.data(), pu.data(), n, (uint32_t)k, tlen);
    return NTC_OK;
}
// test hooks dev_*: device address of a derived array, 0 = not built
int get_dev_addr(const ntc_ctx *ctx, const void *p, int64_t *value) {
    if (!ctx->has_index) return NTC_ERR_NO_INDEX;
    if (hipSetDevice(ctx->device) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) return NTC_ERR_HIP;
    *value = (int64_t)(uintptr_t)p;
    return NTC_OK;
}
// device workspace held now (all slots)
int get_workspace_bytes(const ntc_ctx *ctx, int64_t *value) {
    uint64_t t = 0;
    for (const auto &b : ctx->ws) t += b.bytes;
    *value = (int64_t)t;
    return NTC_OK;
}

#define OPT_SET(member) [](ntc_ctx *c, int64_t v) { c->member = (decltype(c->member))v; return (int)NTC_OK; }
#define OPT_GET(expr) [](const ntc_ctx *c, int64_t *v) { *v = (int64_t)(expr); return (int)NTC_OK; }
// a plain option: get returns what set stored
#define OPT_VALUE(member) OPT_SET(member), OPT_GET(c->member)
// an option of the next ntc_index_upload: get returns what the index in use was built with
#define OPT_UPLOAD(member, built) OPT_SET(member), OPT_GET(c->has_index ? (int64_t)(built) : (int64_t)c->member)
#define OPT_READ(key, expr) {key, 0, 0, kInRange, nullptr, nullptr, OPT_GET(expr)}
#define OPT_DEV(f) {"dev_" #f, 0, 0, kInRange, nullptr, nullptr, \
                    [](const ntc_ctx *c, int64_t *v) { return get_dev_addr(c, c->dix.f, v); }}

constexpr const char *kSmoothMsg = "quality_smooth must be 0 (off) or 12..16777215";
const Option kOptions[] = {
    {"encode_variant", 1, 4, kEndsOnly, "encode_variant must be 4 (default) or 1 (A/B baseline)", OPT_VALUE(encode_variant)},
    {"tab_u", 0, kTabMaxU, kInRange, "tab_u must be 0 (default) or 1..15", OPT_UPLOAD(tab_u_opt, c->dix.tab_u)},
    {"pair_bytes", 0, 1, kInRange, "pair_bytes must be 0 or 1", OPT_UPLOAD(pair_bytes_opt, c->dix.pair_w != nullptr)},
    {"filter", -1, 1, kInRange, "filter must be -1 (auto), 0 or 1", OPT_UPLOAD(filter_opt, c->dix.filt_f != 0)},
    {"joint", -1, 1, kInRange, "joint must be -1 (auto), 0 or 1", OPT_UPLOAD(joint_opt, c->dix.joint)},
    {"path_link", 0, 1, kInRange, "path_link must be 0 or 1", OPT_VALUE(path_link_opt)},
    {"win", -1, 1, kInRange, "win must be -1 (auto), 0 or 1", OPT_UPLOAD(win_opt, c->dix.win_w != nullptr)},
    {"subst", -1, 0, kInRange, "subst must be -1 (auto) or 0", OPT_UPLOAD(subst_opt, c->subst_built)},
    {"uniq_hint", -1, 0, kInRange, "uniq_hint must be -1 (auto) or 0", OPT_UPLOAD(uniq_hint_opt, c->dix.uniq_hint)},
    {"decode_only", 0, 1, kInRange, "decode_only must be 0 or 1", OPT_UPLOAD(decode_only_opt, c->index_decode_only)},
    {"ext2", 0, 1, kInRange, "ext2 must be 0 or 1", OPT_UPLOAD(ext2_opt, c->dix.rank2 != nullptr)},
    {"warm_dma", 1, 1ll << 30, kInRange, "warm_dma: 1 .. 2^30 bytes", warm_dma, nullptr},
    // device workspace ~40 B per base of a pass
    {"max_pass_bases", 1, kNoMax, kInRange, "max_pass_bases must be >= 1", OPT_VALUE(max_pass_bases)},
    // secondary entry slots per read: get returns what 0 (auto) stands for
    {"ent_slots", 0, 1024, kMultipleOf4, "ent_slots must be 0 (auto) or a multiple of 4 up to 1024", OPT_SET(ent_slots_opt),
     OPT_GET(ent_slots(c))},
    {"pool_per_read", 0, kNoMax, kInRange, "pool_per_read must be >= 0", set_pool_per_read, nullptr},
    // the side data of FASTQ and FASTA text (ntcomp_codec.h, ntcomp_gpu.h)
    {"qualities", 0, 2, kInRange, "qualities must be 0 (drop), 1 (keep) or 2 (bin8)", OPT_VALUE(qual.mode)},
    {"quality_coder", 0, 1, kInRange, "quality_coder must be 0 (pack) or 1 (rans)", OPT_VALUE(qual.coder)},
    // smoothing inside long matches: refused at the call when qualities is 0, or when the mode's image of the
    // target does not exceed that of '#'
    {"quality_smooth", 0, kQsMaxM, kInRange, kSmoothMsg,
     [](ntc_ctx *c, int64_t v) {
         if (v && v < kQsMinM) return set_err(c, NTC_ERR_INVALID_ARG, kSmoothMsg);
         c->qual.smooth = (int)v;
         c->qual.smoothed_total = 0;
         return (int)NTC_OK;
     },
     OPT_GET(c->qual.smooth)},
    {"quality_smooth_to", kQsToLo, kQsToHi, kInRange, "quality_smooth_to must be a byte in '$'..'~'", OPT_VALUE(qual.smooth_to)},
    OPT_READ("quality_smoothed", c->qual.smoothed),
    OPT_READ("quality_smoothed_total", c->qual.smoothed_total),  // of the calls since quality_smooth was set: the CLIs' --stats
    {"names", 0, 2, kInRange, "names must be 0 (drop), 1 (keep) or 2 (id)", OPT_VALUE(names.mode)},
    {"discard_text", 0, 1, kInRange, "discard_text must be 0 or 1", OPT_VALUE(discard_text)},
    {"paired", 0, 2, kInRange, "paired must be 0 (off), 1 (ids) or 2 (no check)", OPT_VALUE(pair.mode)},
    {"digests", 0, 1, kInRange, "digests must be 0 or 1", OPT_VALUE(dig.opt)},
    {"gpu_deflate", 0, 1, kInRange, "gpu_deflate must be 0 or 1", OPT_VALUE(df.opt)},
    {"bgzf_text", 0, 1, kInRange, "bgzf_text must be 0 or 1", OPT_VALUE(bz.opt)},
    {"bgzf_workgroups", 0, 65536, kInRange, "bgzf_workgroups must be 0 (two per CU) or 1..65536", OPT_VALUE(bz.workgroups)},
    {"non_acgt", 0, 2, kInRange, "non_acgt must be 0 (error), 1 (mask) or 2 (keep)", OPT_VALUE(nx.policy)},
    // what the last upload and the last calls left
    {"subst_hash", 0, 0, kInRange, nullptr, nullptr, get_subst_hash},
    {"path_hash", 0, 0, kInRange, nullptr, nullptr, get_path_hash},
    {"workspace_bytes", 0, 0, kInRange, nullptr, nullptr, get_workspace_bytes},
    OPT_DEV(walk), OPT_DEV(rank2), OPT_DEV(tab), OPT_DEV(tab_bits),
    OPT_DEV(filt_bits),  // allocated also when filt_f = 0
    OPT_DEV(pair_w), OPT_DEV(win_w),
    OPT_READ("filter_density_ppm", c->filter_density_ppm),
    OPT_READ("n_paths", c->n_paths),
    OPT_READ("path_text_len", c->path_text_len),
    OPT_READ("upload_host_us", c->upload_host_us),
    OPT_READ("upload_total_us", c->upload_total_us),
    OPT_READ("tab_u_fallback", c->tab_u_fallback),
    OPT_READ("pack_us", c->last_pack_ms * 1000.0),
    OPT_READ("spill_reruns", c->spill_reruns),
    OPT_READ("nx_sub", c->has_index ? nx_substitute(c->dix.absent) : 0),
    OPT_READ("nx_runs", c->nx.runs),
    OPT_READ("nx_bases", c->nx.bases),
    OPT_READ("unpack_rice_not_simple", c->unp_path[0]),
    OPT_READ("unpack_rice_serial", c->unp_path[1]),
    OPT_READ("unpack_rice_through", c->unp_path[2]),
    OPT_READ("pool_entries", c->last4.pcap),  // last call's pools
    OPT_READ("pool_records", c->last4.rcap),
};

const Option *find_option(const char *key) {
    for (const Option &o : kOptions)
        if (std::strcmp(key, o.key) == 0) return &o;
    return nullptr;
}
}  // namespace

extern "C" {

int ntc_ctx_set_option(ntc_ctx *ctx, const char *key, int64_t value) {
    if (!ctx || !key) return NTC_ERR_INVALID_ARG;
    const Option *o = find_option(key);
    if (!o || !o->set) return set_err(ctx, NTC_ERR_INVALID_ARG, std::string("unknown option ") + key);
    if (value < o->lo || value > o->hi || (o->rule == kEndsOnly && value != o->lo && value != o->hi) ||
        (o->rule == kMultipleOf4 && (value & 3)))
        return set_err(ctx, NTC_ERR_INVALID_ARG, o->msg);
    return o->set(ctx, value);
}

int ntc_ctx_get_option(const ntc_ctx *ctx, const char *key, int64_t *value) {
    if (!ctx || !key || !value) return NTC_ERR_INVALID_ARG;
    const Option *o = find_option(key);
    return o && o->get ? o->get(ctx, value) : NTC_ERR_INVALID_ARG;
}

int ntc_index_info(const ntc_ctx *ctx, uint64_t *n_nodes, uint32_t *k, uint64_t *device_bytes) {
    if (!ctx) return NTC_ERR_INVALID_ARG;
    if (!ctx->has_index) return NTC_ERR_NO_INDEX;
    if (n_nodes) *n_nodes = ctx->dix.n;
    if (k) *k = ctx->dix.k;
    if (device_bytes) *device_bytes = ctx->index_bytes;
    return NTC_OK;
}

int ntc_encode_batch_device(ntc_ctx *ctx, const uint8_t *d_bases, const uint64_t *d_read_offsets,
                            uint64_t n_reads, uint32_t max_read_len, uint64_t *d_rec_out,
                            uint64_t rec_capacity, uint64_t *d_rec_offsets_out) {
    if (!ctx || (!d_read_offsets && n_reads) || !d_rec_offsets_out)
        return set_err(ctx, NTC_ERR_INVALID_ARG, "null argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (ctx->qual.mode != 0) return q_unsupported(ctx, "ntc_encode_batch_device");
    if (ctx->names.mode != 0) return n_unsupported(ctx, "ntc_encode_batch_device");
    if (ctx->nx.policy != 0)
        return set_err(ctx, NTC_ERR_UNSUPPORTED, "non_acgt mask / keep need the host-buffer encode calls "
                                                 "(the caller's device buffer is const)");
    if (ctx->encode_variant == 4) {
        if (!ctx->has_index) return set_err(ctx, NTC_ERR_NO_INDEX, "no index uploaded");
        uint64_t total = 0;
        if (n_reads) {
            if (max_read_len > 0) {
                total = n_reads * (uint64_t)max_read_len;  // an upper bound is enough
            } else {
                uint64_t ends[2] = {0, 0};
                HIP_TRY(ctx, hipMemcpyAsync(&ends[0], d_read_offsets, 8, hipMemcpyDeviceToHost, ctx->stream));
                HIP_TRY(ctx, hipMemcpyAsync(&ends[1], d_read_offsets + n_reads, 8, hipMemcpyDeviceToHost, ctx->stream));
                HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
                total = ends[1] - ends[0];
            }
        }
        return encode4_impl(ctx, d_bases, d_read_offsets, n_reads, total, d_rec_out, rec_capacity,
                            d_rec_offsets_out);
    }
    Layout lay;
    const uint64_t tiles = (n_reads + 63) / 64;
    if (max_read_len > 0) {
        lay.rows_uniform = ((uint64_t)max_read_len + 31) & ~31ULL;
        lay.total_rows = tiles * lay.rows_uniform;
    } else if (n_reads > 0) {
        void *rows, *tb, *tmp;
        int rc;
        if ((rc = ensure(ctx, WS_TILEROWS, tiles * 4, &rows))) return rc;
        if ((rc = ensure(ctx, WS_TILEBASE, (tiles + 1) * 8, &tb))) return rc;
        if ((rc = ensure(ctx, WS_SCANTMP, scan_tmp_words(std::max(tiles, n_reads) + 1) * 8, &tmp)))
            return rc;
        launch_tile_rows(d_read_offsets, n_reads, (uint32_t *)rows, ctx->stream);
        scan_excl_u32((const uint32_t *)rows, tiles, (uint64_t *)tb, (uint64_t *)tmp, ctx->stream);
        HIP_TRY(ctx, hipMemcpyAsync(&lay.total_rows, (uint64_t *)tb + tiles, 8, hipMemcpyDeviceToHost,
                                    ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        lay.d_tile_base = (const uint64_t *)tb;
    }
    return encode_impl(ctx, d_bases, d_read_offsets, n_reads, lay, d_rec_out, rec_capacity,
                       d_rec_offsets_out, 0);
}

int ntc_encode_status(ntc_ctx *ctx, int64_t *bad_read, uint64_t *n_records) {
    if (!ctx) return NTC_ERR_INVALID_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = read_status(ctx, bad_read);
    if (rc) return rc;
    if (n_records) {
        if (ctx->last != kEncode || !ctx->last_out_offs) return set_err(ctx, NTC_ERR_INVALID_ARG, "no encode call");
        if (ctx->box_valid) *n_records = box(ctx, kBoxA);
        else HIP_TRY(ctx, hipMemcpy(n_records, ctx->last_out_offs + ctx->last_n, 8, hipMemcpyDeviceToHost));
    }
    return NTC_OK;
}

namespace {
// one device pass of the v1 (A/B baseline) encoder over all reads
int encode_batch_v1(ntc_ctx *ctx, const uint8_t *bases, const uint64_t *read_offsets, uint64_t n_reads,
                    uint64_t *rec_out, uint64_t rec_capacity, uint64_t *rec_offsets_out, int64_t *bad_read) {
    const uint64_t o0 = read_offsets[0], total = read_offsets[n_reads] - o0;
    // per-tile scratch rows (host knows every length)
    const uint64_t tiles = (n_reads + 63) / 64;
    std::vector<uint64_t> tb(tiles + 1, 0), offs(n_reads + 1);
    for (uint64_t t = 0; t < tiles; t++) {
        uint64_t mx = 0;
        for (uint64_t r = t * 64; r < std::min(n_reads, t * 64 + 64); r++)
            mx = std::max(mx, read_offsets[r + 1] - read_offsets[r]);
        tb[t + 1] = tb[t] + ((mx + 31) & ~31ULL);
    }
    for (uint64_t r = 0; r <= n_reads; r++) offs[r] = read_offsets[r] - o0;
    void *d_bases, *d_offs, *d_tb, *d_recs, *d_roffs;
    int rc;
    if ((rc = ensure(ctx, WS_STAGE_BASES, total + 64, &d_bases))) return rc;
    if ((rc = ensure(ctx, WS_STAGE_OFFS, (n_reads + 1) * 8 * 2, &d_offs))) return rc;
    if ((rc = ensure(ctx, WS_TILEBASE, (tiles + 1) * 8, &d_tb))) return rc;
    if ((rc = ensure(ctx, WS_STAGE_RECS, (total + 1) * 8, &d_recs))) return rc;
    d_roffs = (uint64_t *)d_offs + (n_reads + 1);
    if (total) HIP_TRY(ctx, hipMemcpyAsync(d_bases, bases + o0, total, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d_offs, offs.data(), (n_reads + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d_tb, tb.data(), (tiles + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    Layout lay;
    lay.d_tile_base = (const uint64_t *)d_tb;
    lay.total_rows = tb[tiles];
    rc = encode_impl(ctx, (const uint8_t *)d_bases, (const uint64_t *)d_offs, n_reads, lay, (uint64_t *)d_recs,
                     total + 1, (uint64_t *)d_roffs, total);
    if (rc) return rc;
    rc = read_status(ctx, bad_read);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpy(rec_offsets_out, d_roffs, (n_reads + 1) * 8, hipMemcpyDeviceToHost));
    const uint64_t nrec = rec_offsets_out[n_reads];
    if (nrec > rec_capacity) return set_err(ctx, NTC_ERR_CAPACITY, "rec_capacity smaller than the number of records");
    if (nrec) HIP_TRY(ctx, hipMemcpy(rec_out, d_recs, nrec * 8, hipMemcpyDeviceToHost));
    return NTC_OK;
}
}  // namespace

int ntc_encode_batch(ntc_ctx *ctx, const uint8_t *bases, const uint64_t *read_offsets, uint64_t n_reads,
                     uint64_t *rec_out, uint64_t rec_capacity, uint64_t *rec_offsets_out, int64_t *bad_read) {
    if (bad_read) *bad_read = -1;
    if (!ctx || !read_offsets || !rec_offsets_out || (n_reads && !bases))
        return set_err(ctx, NTC_ERR_INVALID_ARG, "null argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    for (uint64_t r = 0; r < n_reads; r++)
        if (read_offsets[r + 1] < read_offsets[r])
            return set_err(ctx, NTC_ERR_INVALID_ARG, "read offsets must be non-decreasing");
    if (!ctx->has_index) return set_err(ctx, NTC_ERR_NO_INDEX, "no index uploaded");
    if (ctx->qual.mode != 0) return q_unsupported(ctx, "ntc_encode_batch");
    if (ctx->names.mode != 0) return n_unsupported(ctx, "ntc_encode_batch");
    ctx->nx.begin();
    if (ctx->encode_variant != 4 && ctx->nx.policy != 0)
        return set_err(ctx, NTC_ERR_UNSUPPORTED, "non_acgt mask / keep need encode_variant 4");
    if (ctx->encode_variant != 4)
        return encode_batch_v1(ctx, bases, read_offsets, n_reads, rec_out, rec_capacity, rec_offsets_out, bad_read);
    // passes of whole reads, at most max_pass_bases each (one read may exceed it alone), so
    // the device workspace stays bounded however large the host batch is
    std::vector<uint64_t> offs, roffs;
    uint64_t r0 = 0, produced = 0;
    rec_offsets_out[0] = 0;
    do {
        uint64_t r1 = std::min(n_reads, r0 + 1);
        if (r1 < n_reads) {  // largest r1 with bases [r0, r1) <= max_pass_bases
            uint64_t lo = r1, hi = n_reads;
            while (lo < hi) {
                const uint64_t mid = (lo + hi + 1) / 2;
                if (read_offsets[mid] - read_offsets[r0] <= ctx->max_pass_bases) lo = mid;
                else hi = mid - 1;
            }
            r1 = lo;
        }
        const uint64_t nr = r1 - r0, o0 = read_offsets[r0], total = read_offsets[r1] - o0;
        offs.resize(nr + 1);
        for (uint64_t r = 0; r <= nr; r++) offs[r] = read_offsets[r0 + r] - o0;
        void *d_bases, *d_offs, *d_recs;
        int rc;
        if ((rc = ensure(ctx, WS_STAGE_BASES, total + 64, &d_bases))) return rc;
        if ((rc = ensure(ctx, WS_STAGE_OFFS, (nr + 1) * 8 * 2, &d_offs))) return rc;
        if ((rc = ensure(ctx, WS_STAGE_RECS, (total + 1) * 8, &d_recs))) return rc;
        uint64_t *d_roffs = (uint64_t *)d_offs + (nr + 1);
        HIP_TRY(ctx, hipMemcpyAsync(d_offs, offs.data(), (nr + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
        for (bool again = true; again;) {  // twice only when the pass holds more runs than the list had room for
            if (total) HIP_TRY(ctx, hipMemcpyAsync(d_bases, bases + o0, total, hipMemcpyHostToDevice, ctx->stream));
            if ((rc = nx_mask(ctx, (uint8_t *)d_bases, (const uint64_t *)d_offs, nr, total))) return rc;
            rc = encode4_impl(ctx, (const uint8_t *)d_bases, (const uint64_t *)d_offs, nr, total, (uint64_t *)d_recs,
                              total + 1, d_roffs);
            if (rc) return rc;
            int64_t bad = -1;
            rc = read_status(ctx, &bad);
            if (rc) {
                if (bad_read) *bad_read = bad + (int64_t)r0;
                char buf[160];
                std::snprintf(buf, sizeof(buf), "%s at index %lld", status_name(rc), (long long)(bad + (int64_t)r0));
                ctx->err = buf;
                return rc;
            }
            if ((rc = nx_collect(ctx, r0, &again))) return rc;
        }
        roffs.resize(nr + 1);
        HIP_TRY(ctx, hipMemcpy(roffs.data(), d_roffs, (nr + 1) * 8, hipMemcpyDeviceToHost));
        const uint64_t nrec = roffs[nr];
        if (produced + nrec > rec_capacity)
            return set_err(ctx, NTC_ERR_CAPACITY, "rec_capacity smaller than the number of records");
        for (uint64_t r = 1; r <= nr; r++) rec_offsets_out[r0 + r] = produced + roffs[r];
        if (nrec) HIP_TRY(ctx, hipMemcpy(rec_out + produced, d_recs, nrec * 8, hipMemcpyDeviceToHost));
        produced += nrec;
        r0 = r1;
    } while (r0 < n_reads);
    return NTC_OK;
}

int ntc_decode_batch_device(ntc_ctx *ctx, const uint64_t *d_recs, uint64_t n_recs, uint8_t *d_bases_out,
                            uint64_t bases_capacity, uint64_t *d_read_offsets_out, uint64_t offsets_capacity) {
    if (!ctx || (!d_recs && n_recs) || !d_read_offsets_out) return set_err(ctx, NTC_ERR_INVALID_ARG, "null argument");
    if (!ctx->has_index) return set_err(ctx, NTC_ERR_NO_INDEX, "no index uploaded");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    void *ws, *tmp;
    int rc;
    const uint64_t n = n_recs;
    // per kDecTileRecs-record tile: pf, pl (sums) then pfs, pls (exclusive scans, totals at [tiles])
    const uint64_t tiles = (n + kDecTileRecs - 1) / kDecTileRecs;
    if ((rc = ensure(ctx, WS_DEC_C, (4 * tiles + 2) * 8, &ws))) return rc;
    uint64_t *pf = (uint64_t *)ws, *pl = pf + tiles, *pfs = pl + tiles, *pls = pfs + tiles + 1;
    if ((rc = ensure(ctx, WS_SCANTMP, (scan_tmp_words(tiles + 1) + 2) * 8, &tmp))) return rc;
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_status, 0xFF, 8, ctx->stream));
    ctx->box_valid = false;
    ctx->last = kDecode;
    ctx->last_n = tiles;
    ctx->last_out_offs = pfs;  // pfs[tiles] = reads, pls[tiles] = bases (ntc_decode_status)
    HIP_TRY(ctx, hipEventRecord(ctx->ev[0], ctx->stream));
    if (n == 0) {
        HIP_TRY(ctx, hipMemsetAsync(pfs, 0, 16, ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(d_read_offsets_out, 0, 8, ctx->stream));
        for (int i = 1; i < 4; i++) HIP_TRY(ctx, hipEventRecord(ctx->ev[i], ctx->stream));
        return NTC_OK;
    }
    launch_dec_tiles(d_recs, n, pf, pl, pfs, pls, (uint64_t *)tmp, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ctx->ev[1], ctx->stream));
    DecWalkArgs wa{};
    wa.ix = ctx->dix;
    wa.recs = d_recs;
    wa.n = n;
    wa.pfs = pfs;
    wa.pls = pls;
    wa.offs_out = d_read_offsets_out;
    wa.offs_capacity = offsets_capacity;
    wa.bases_capacity = bases_capacity;
    wa.out = d_bases_out;
    wa.status = ctx->d_status;
    launch_dec_walk(wa, ctx->stream);
    HIP_TRY(ctx, hipEventRecord(ctx->ev[3], ctx->stream));  // k_dec_rec alone: ev[1] -> ev[3]
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ctx->ev[2], ctx->stream));
    launch_status_box(ctx->d_status, pfs + tiles, pls + tiles, nullptr, ctx->h_box, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    ctx->box_valid = true;
    return NTC_OK;
}

int ntc_decode_status(ntc_ctx *ctx, uint64_t *n_reads, uint64_t *n_bases) {
    if (!ctx) return NTC_ERR_INVALID_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = read_status(ctx, nullptr);
    if (ctx->last != kDecode) return set_err(ctx, NTC_ERR_INVALID_ARG, "no decode call");
    uint64_t nr = 0, nb = 0;
    if (ctx->box_valid) {
        nr = box(ctx, kBoxA);
        nb = box(ctx, kBoxB);
    } else {
        HIP_TRY(ctx, hipMemcpy(&nr, ctx->last_out_offs + ctx->last_n, 8, hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(&nb, ctx->last_out_offs + (ctx->last_n + 1) + ctx->last_n, 8, hipMemcpyDeviceToHost));
    }
    if (n_reads) *n_reads = nr;
    if (n_bases) *n_bases = nb;
    ctx->last_units = nb;
    return rc;
}

int ntc_decode_batch(ntc_ctx *ctx, const uint64_t *recs, uint64_t n_recs, uint8_t *bases_out,
                     uint64_t bases_capacity, uint64_t *read_offsets_out, uint64_t offsets_capacity,
                     uint64_t *n_reads_out, uint64_t *n_bases_out) {
    if (!ctx || (!recs && n_recs)) return set_err(ctx, NTC_ERR_INVALID_ARG, "null argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    uint64_t nreads = 0, nbases = 0;
    for (uint64_t r = 0; r < n_recs; r++) {
        const uint32_t flag = (uint32_t)(recs[r] >> 56);
        nreads += flag & 1;
        nbases += (flag & 2) ? (flag >> 2) : ((uint32_t)(recs[r] >> 32) & 0xFFFFFFu);
    }
    if (n_reads_out) *n_reads_out = nreads;
    if (n_bases_out) *n_bases_out = nbases;
    if (n_recs && !((recs[0] >> 56) & 1)) return set_err(ctx, NTC_ERR_FORMAT, "records do not start a read");
    if (nbases > bases_capacity || nreads + 1 > offsets_capacity || !read_offsets_out || (nbases && !bases_out))
        return set_err(ctx, NTC_ERR_CAPACITY, "decode output buffers too small");
    Pending<ntc_nx_run> nxp;  // pending exception runs: each pass patches its own reads'
    const bool has_nx = ctx->nx.pending.take(nxp);
    const std::vector<ntc_nx_run> &nx = nxp.metas;
    const uint32_t nx_sub = ctx->nx.pending_sub;
    if (has_nx && nx.back().read >= nreads) return set_err(ctx, NTC_ERR_FORMAT, "exception run past the last read");
    // passes of whole reads (a pass ends before a `first` record), at most max_pass_bases
    // output bases each unless one read alone is larger
    uint64_t a0 = 0, reads_done = 0, bases_done = 0;
    read_offsets_out[0] = 0;
    std::vector<uint64_t> offs;
    while (a0 < n_recs) {
        uint64_t a1 = a0, pb = 0, pr = 0;
        while (a1 < n_recs) {
            const uint32_t flag = (uint32_t)(recs[a1] >> 56);
            const uint64_t len = (flag & 2) ? (flag >> 2) : ((uint32_t)(recs[a1] >> 32) & 0xFFFFFFu);
            if ((flag & 1) && a1 > a0 && pb + len > ctx->max_pass_bases) break;
            pb += len;
            pr += flag & 1;
            a1++;
        }
        // a read runs to the next `first` record: extend the pass over the rest of this read
        while (a1 < n_recs && !((recs[a1] >> 56) & 1)) {
            const uint32_t flag = (uint32_t)(recs[a1] >> 56);
            pb += (flag & 2) ? (flag >> 2) : ((uint32_t)(recs[a1] >> 32) & 0xFFFFFFu);
            a1++;
        }
        const uint64_t nrec = a1 - a0;
        void *d_recs, *d_out, *d_offs;
        int rc;
        if ((rc = ensure(ctx, WS_STAGE_RECS, (nrec + 1) * 8, &d_recs))) return rc;
        if ((rc = ensure(ctx, WS_STAGE_BASES, pb + 64, &d_out))) return rc;
        if ((rc = ensure(ctx, WS_STAGE_OFFS, (pr + 1) * 8, &d_offs))) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(d_recs, recs + a0, nrec * 8, hipMemcpyHostToDevice, ctx->stream));
        rc = ntc_decode_batch_device(ctx, (const uint64_t *)d_recs, nrec, (uint8_t *)d_out, pb, (uint64_t *)d_offs,
                                     pr + 1);
        if (rc) return rc;
        if (!nx.empty() && (rc = nx_patch(ctx, nx, nx_sub, reads_done, pr, (uint8_t *)d_out, (const uint64_t *)d_offs)))
            return rc;
        uint64_t nr = 0, nb = 0;
        rc = ntc_decode_status(ctx, &nr, &nb);
        if (rc) return rc;
        if (nr != pr || nb != pb) return set_err(ctx, NTC_ERR_FORMAT, "decode size mismatch");
        offs.resize(pr + 1);
        HIP_TRY(ctx, hipMemcpy(offs.data(), d_offs, (pr + 1) * 8, hipMemcpyDeviceToHost));
        for (uint64_t r = 1; r <= pr; r++) read_offsets_out[reads_done + r] = bases_done + offs[r];
        if (pb) HIP_TRY(ctx, hipMemcpy(bases_out + bases_done, d_out, pb, hipMemcpyDeviceToHost));
        reads_done += pr;
        bases_done += pb;
        a0 = a1;
    }
    return NTC_OK;
}

int ntc_pack_blocks_device(ntc_ctx *ctx, const uint64_t *d_recs, const uint64_t *d_rec_offsets,
                           uint64_t n_reads, uint32_t block_reads, uint8_t *d_payload,
                           uint64_t payload_capacity, ntc_block_meta *meta, uint64_t *payload_bytes) {
    if (!ctx || !d_rec_offsets || !meta || !payload_bytes || block_reads == 0 || (n_reads && (!d_recs || !d_payload)))
        return set_err(ctx, NTC_ERR_INVALID_ARG, "null argument or block_reads = 0");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return pack_blocks_impl(ctx, d_recs, d_rec_offsets, n_reads, block_reads, d_payload, payload_capacity, meta,
                            payload_bytes);
}

}  // extern "C"

namespace {
// The members of n_blocks packed blocks (deflate.hip): d_payload as the packer left it, metas on
// the host.  member_off_len: 4 pairs per block of where a stream's member starts in d_out and
// its bytes (zeros for a block whose status is not 0).  *out_bytes: the bytes used, or with
// NTC_ERR_CAPACITY the bytes needed: the sum of the members' bounds, which needs no device pass.
int deflate_blocks_impl(ntc_ctx *ctx, const uint8_t *d_payload, const ntc_block_meta *metas, uint64_t n_blocks,
                        uint8_t *d_out, uint64_t out_capacity, uint64_t *member_off_len, uint64_t *out_bytes) {
    DeflateState &D = ctx->df;
    D.chunks.clear();
    D.streams.clear();
    uint64_t need = 0;
    for (uint64_t b = 0; b < n_blocks; b++) {
        if (metas[b].status != NTC_OK) continue;
        for (int s = 0; s < 4; s++) {
            const ntc_stream_meta &m = metas[b].stream[s];
            if (m.encoded_size >> 28) return set_err(ctx, NTC_ERR_INVALID_ARG, "a stream of 2 GiB or more");
            const uint64_t n = m.encoded_size * 8, nc = df_chunks(n);
            if ((D.chunks.size() + nc) >> 31) return set_err(ctx, NTC_ERR_CAPACITY, "too many chunks in one call: split the batch");
            D.streams.push_back(DfStreamDesc{n, (uint32_t)D.chunks.size(), (uint32_t)nc});
            for (uint64_t c = 0; c < nc; c++) {
                const uint64_t off = c * kDfChunk;
                D.chunks.push_back(DfChunkDesc{m.offset + off, (uint32_t)std::min<uint64_t>(n - off, kDfChunk), c + 1 == nc});
            }
            need += df_member_bound(n);
        }
    }
    *out_bytes = need;
    if (need > out_capacity)
        return set_err(ctx, NTC_ERR_CAPACITY, "deflate output needs " + std::to_string(need) + " bytes");
    for (uint64_t i = 0; i < n_blocks * 8; i++) member_off_len[i] = 0;
    *out_bytes = 0;
    const uint64_t N = D.chunks.size(), S = D.streams.size();
    if (!S) return NTC_OK;
    void *d_desc, *d_tokens, *d_stage, *d_res;
    int rc;
    const uint64_t res_bytes = N * sizeof(DfResult) + N * 8 + (2 * S + 1) * 8 + S * 4;
    if ((rc = ensure(ctx, WS_DF_DESC, N * sizeof(DfChunkDesc) + S * sizeof(DfStreamDesc), &d_desc))) return rc;
    if ((rc = ensure(ctx, WS_DF_TOKENS, N * kDfChunk * 4, &d_tokens))) return rc;
    if ((rc = ensure(ctx, WS_DF_STAGE, N * kDfSlot, &d_stage))) return rc;
    if ((rc = ensure(ctx, WS_DF_RES, res_bytes, &d_res))) return rc;
    DfArgs a{};
    a.payload = d_payload;
    a.chunks = (const DfChunkDesc *)d_desc;
    a.streams = (const DfStreamDesc *)(a.chunks + N);
    a.n_chunks = (uint32_t)N;
    a.n_streams = (uint32_t)S;
    a.tokens = (uint32_t *)d_tokens;
    a.stage = (uint8_t *)d_stage;
    a.results = (DfResult *)d_res;
    a.chunk_off = (uint64_t *)(a.results + N);
    a.member_off_len = a.chunk_off + N;
    a.crcs = (uint32_t *)(a.member_off_len + 2 * S + 1);
    a.out = d_out;
    HIP_TRY(ctx, hipMemcpyAsync(d_desc, D.chunks.data(), N * sizeof(DfChunkDesc), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync((void *)a.streams, D.streams.data(), S * sizeof(DfStreamDesc), hipMemcpyHostToDevice,
                                ctx->stream));
    launch_deflate(a, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    D.dev_off_len.resize(2 * S + 1);
    HIP_TRY(ctx, hipMemcpyAsync(D.dev_off_len.data(), a.member_off_len, (2 * S + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    uint64_t s = 0;
    for (uint64_t b = 0; b < n_blocks; b++) {
        if (metas[b].status != NTC_OK) continue;
        for (int k = 0; k < 8; k++) member_off_len[b * 8 + k] = D.dev_off_len[2 * s + k];
        s += 4;
    }
    *out_bytes = D.dev_off_len[2 * S];
    return NTC_OK;
}
}  // namespace

extern "C" {

int ntc_deflate_blocks_device(ntc_ctx *ctx, const uint8_t *d_payload, const ntc_block_meta *metas, uint64_t n_blocks,
                              uint8_t *d_out, uint64_t out_capacity, uint64_t *member_off_len, uint64_t *out_bytes) {
    if (!ctx || !out_bytes || (n_blocks && (!metas || !member_off_len)))
        return set_err(ctx, NTC_ERR_INVALID_ARG, "null argument");
    *out_bytes = 0;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    for (uint64_t b = 0; b < n_blocks; b++)
        if (metas[b].status == NTC_OK && (!d_payload || !d_out))
            return set_err(ctx, NTC_ERR_INVALID_ARG, "null device buffer");
    return deflate_blocks_impl(ctx, d_payload, metas, n_blocks, d_out, out_capacity, member_off_len, out_bytes);
}

int ntc_encode_members(ntc_ctx *ctx, uint64_t *member_off_len, uint64_t cap_blocks, uint64_t *n_blocks) {
    if (!ctx || !n_blocks) return set_err(ctx, NTC_ERR_INVALID_ARG, "null argument");
    *n_blocks = ctx->df.members.size() / 8;
    if (*n_blocks > cap_blocks || (*n_blocks && !member_off_len))
        return set_err(ctx, NTC_ERR_CAPACITY, "member array too small");
    std::copy(ctx->df.members.begin(), ctx->df.members.end(), member_off_len);
    return NTC_OK;
}

}  // extern "C"

// ---- inflate of gzip members (inflate.hip) ----------------------------------------------------
namespace {
static_assert(sizeof(ntc_inflate_member) == 24 && sizeof(InfMemberDesc) == 24 && offsetof(ntc_inflate_member, dst_off) == 16 &&
                  offsetof(InfMemberDesc, dst_off) == 16 && offsetof(InfMemberDesc, out_bytes) == 12,
              "ntc_inflate_member is the kernel's descriptor");
static_assert(sizeof(ntc_inflate_result) == sizeof(InfResult) && NTC_INFLATE_MAX_OUT == kInfMaxOut, "ntc_inflate_result is the kernel's result");

// What ntc_inflate_members refuses before anything runs.  order: the members with bytes to
// write, by dst_off; span: [0] / [1] the first and one past the last byte of comp they cover,
// [2] / [3] the same of dst.
int inflate_check(ntc_ctx *ctx, uint64_t comp_bytes, const ntc_inflate_member *m, uint64_t n, uint64_t dst_cap,
                  std::vector<uint32_t> &order, uint64_t span[4]) {
    if (n >> 31) return set_err(ctx, NTC_ERR_INVALID_ARG, "2^31 members or more in one call");
    span[0] = span[2] = UINT64_MAX, span[1] = span[3] = 0;
    order.clear();
    for (uint64_t i = 0; i < n; i++) {
        if (m[i].src_off > comp_bytes || m[i].src_bytes > comp_bytes - m[i].src_off)
            return set_err(ctx, NTC_ERR_INVALID_ARG, "member " + std::to_string(i) + " lies outside the compressed bytes");
        if (m[i].dst_off > dst_cap || m[i].out_bytes > dst_cap - m[i].dst_off)
            return set_err(ctx, NTC_ERR_INVALID_ARG, "member " + std::to_string(i) + " lies outside the output");
        span[0] = std::min(span[0], m[i].src_off), span[1] = std::max(span[1], m[i].src_off + m[i].src_bytes);
        span[2] = std::min(span[2], m[i].dst_off), span[3] = std::max(span[3], m[i].dst_off + m[i].out_bytes);
        if (m[i].out_bytes) order.push_back((uint32_t)i);
    }
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return m[a].dst_off < m[b].dst_off; });
    for (size_t k = 1; k < order.size(); k++)
        if (m[order[k - 1]].dst_off + m[order[k - 1]].out_bytes > m[order[k]].dst_off)
            return set_err(ctx, NTC_ERR_INVALID_ARG, "members " + std::to_string(order[k - 1]) + " and " +
                                                         std::to_string(order[k]) + " overlap in the output");
    if (!n) span[0] = span[2] = 0;
    return NTC_OK;
}

// descriptors up, the kernel, results down (device buffers d_comp / d_dst; the descriptors'
// offsets less src_base / dst_base)
int inflate_launch(ntc_ctx *ctx, const uint8_t *d_comp, uint64_t src_base, const ntc_inflate_member *m, uint64_t n,
                   uint8_t *d_dst, uint64_t dst_base, ntc_inflate_result *res) {
    void *d_desc, *d_res;
    int rc;
    if ((rc = ensure(ctx, WS_INF_DESC, n * sizeof(InfMemberDesc), &d_desc))) return rc;
    if ((rc = ensure(ctx, WS_INF_RES, n * sizeof(InfResult), &d_res))) return rc;
    std::vector<InfMemberDesc> desc(n);
    for (uint64_t i = 0; i < n; i++)
        desc[i] = InfMemberDesc{m[i].src_off - src_base, m[i].src_bytes, m[i].out_bytes, m[i].dst_off - dst_base};
    HIP_TRY(ctx, hipMemcpyAsync(d_desc, desc.data(), n * sizeof(InfMemberDesc), hipMemcpyHostToDevice, ctx->stream));
    InfArgs a{};
    a.comp = d_comp;
    a.members = (const InfMemberDesc *)d_desc;
    a.n_members = (uint32_t)n;
    a.dst = d_dst;
    a.results = (InfResult *)d_res;
    launch_inflate(a, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(res, d_res, n * sizeof(InfResult), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (desc lives until here)
    return NTC_OK;
}
}  // namespace

extern "C" {

int ntc_inflate_members(ntc_ctx *ctx, const uint8_t *comp, uint64_t comp_bytes, const ntc_inflate_member *m, uint64_t n,
                        uint8_t *dst, uint64_t dst_cap, ntc_inflate_result *res, uint64_t *n_failed) {
    if (!n_failed || (n && (!m || !res || !comp))) return set_err(ctx, NTC_ERR_INVALID_ARG, "null argument");
    *n_failed = 0;
    std::vector<uint32_t> order;
    uint64_t span[4];
    int rc;
    if ((rc = inflate_check(ctx, comp_bytes, m, n, dst_cap, order, span))) return rc;
    if (!order.empty() && !dst) return set_err(ctx, NTC_ERR_INVALID_ARG, "null argument");
    if (!n) return NTC_OK;
    if (!ctx) {  // the host restatement: the kernel's function, one lane
        InfWork *W = new InfWork;
        for (uint64_t i = 0; i < n; i++) {
            inf_member(W, comp + m[i].src_off, m[i].src_bytes, m[i].out_bytes, dst + m[i].dst_off, (InfResult *)&res[i], 0, 1);
            *n_failed += res[i].status != 0;
        }
        delete W;
        return NTC_OK;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // the compressed bytes the members cover go up; the output's place starts 16-aligned so that
    // a member lands as aligned on the device as it will on the host
    const uint64_t dst_base = span[2] & ~15ull;
    void *d_comp, *d_dst;
    if ((rc = ensure(ctx, WS_INF_COMP, span[1] - span[0], &d_comp))) return rc;
    if ((rc = ensure(ctx, WS_INF_DST, span[3] - dst_base, &d_dst))) return rc;
    if (span[1] > span[0])
        HIP_TRY(ctx, hipMemcpyAsync(d_comp, comp + span[0], span[1] - span[0], hipMemcpyHostToDevice, ctx->stream));
    if ((rc = inflate_launch(ctx, (const uint8_t *)d_comp, span[0], m, n, (uint8_t *)d_dst, dst_base, res))) return rc;
    for (uint64_t i = 0; i < n; i++) *n_failed += res[i].status != 0;
    // the sound members' bytes come down, neighbours in one copy; nothing else of dst is touched
    for (size_t k = 0; k < order.size();) {
        if (res[order[k]].status) {
            k++;
            continue;
        }
        const uint64_t from = m[order[k]].dst_off;
        uint64_t to = from + m[order[k]].out_bytes;
        for (k++; k < order.size() && !res[order[k]].status && m[order[k]].dst_off == to; k++) to += m[order[k]].out_bytes;
        HIP_TRY(ctx, hipMemcpyAsync(dst + from, (const uint8_t *)d_dst + (from - dst_base), to - from, hipMemcpyDeviceToHost,
                                    ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return NTC_OK;
}

int ntc_inflate_members_device(ntc_ctx *ctx, const void *d_comp, uint64_t comp_bytes, const ntc_inflate_member *m,
                               uint64_t n, void *d_dst, uint64_t dst_cap, ntc_inflate_result *res, uint64_t *n_failed) {
    if (!ctx || !n_failed || (n && (!m || !res || !d_comp))) return set_err(ctx, NTC_ERR_INVALID_ARG, "null argument");
    *n_failed = 0;
    std::vector<uint32_t> order;
    uint64_t span[4];
    int rc;
    if ((rc = inflate_check(ctx, comp_bytes, m, n, dst_cap, order, span))) return rc;
    if (!order.empty() && !d_dst) return set_err(ctx, NTC_ERR_INVALID_ARG, "null argument");
    if (!n) return NTC_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = inflate_launch(ctx, (const uint8_t *)d_comp, 0, m, n, (uint8_t *)d_dst, 0, res))) return rc;
    for (uint64_t i = 0; i < n; i++) *n_failed += res[i].status != 0;
    return NTC_OK;
}

}  // extern "C"

// ---- BGZF members of a text (bgzf.hip, bgzf_core.h) ---------------------------------------------
namespace {
static_assert(sizeof(ntc_bgzf_member) == sizeof(BgzfMember) && offsetof(ntc_bgzf_member, place) == offsetof(BgzfMember, place),
              "ntc_bgzf_member is the kernel's member table entry");

// The members of the n bytes at d_text into d_out (room for bgzf_bound(n) bytes), all device
// memory.  d_off (null: plain cuts): n_rec + 1 offsets, d_off[r] - off_base being record r's
// start.  The table is appended to tab with the places moved by place_base, the counts are added
// to counts.  One wait between the plan and the coder (the chunk count), one at the end.
int bgzf_dev(ntc_ctx *ctx, const uint8_t *d_text, uint64_t n, const uint64_t *d_off, uint64_t n_rec, uint64_t off_base,
             uint8_t *d_out, uint64_t place_base, std::vector<BgzfMember> &tab, uint64_t counts[7]) {
    if (n == 0) return NTC_OK;
    if (n >> 32) return set_err(ctx, NTC_ERR_CAPACITY, "4 GiB of text or more in one BGZF call: split the batch");
    const uint64_t C = bgzf_cells(n, d_off != nullptr), M = bgzf_members_max(n), N = M * kBgzfMemberChunks;
    const uint32_t wgs = ctx->bz.workgroups ? (uint32_t)ctx->bz.workgroups : (uint32_t)std::max(1, 2 * ctx->num_cus);
    const auto up = [](uint64_t b) { return (b + 15) & ~15ull; };
    const uint64_t b_cuts = up((C + 1) * 8), b_members = up(M * sizeof(BgzfMember)), b_m32 = up(M * 4),
                   b_chunks = up(N * sizeof(DfChunkDesc)), b_res = up(N * sizeof(DfResult)), b_coff = up(N * 8);
    void *d_plan, *d_tokens, *d_stage;
    int rc;
    if ((rc = ensure(ctx, WS_BZ_PLAN, 64 + 2 * b_cuts + b_members + 2 * b_m32 + b_chunks + b_res + b_coff, &d_plan))) return rc;
    if ((rc = ensure(ctx, WS_BZ_TOKENS, (uint64_t)wgs * kDfChunk * 4, &d_tokens))) return rc;
    if ((rc = ensure(ctx, WS_BZ_STAGE, N * kDfSlot, &d_stage))) return rc;
    BgzfArgs a{};
    uint8_t *p = (uint8_t *)d_plan;
    const auto take = [&p](uint64_t b) {
        uint8_t *q = p;
        p += b;
        return q;
    };
    a.counts = (uint64_t *)take(64);
    a.cuts = (uint64_t *)take(b_cuts);
    a.cell_first = (uint64_t *)take(b_cuts);
    a.members = (BgzfMember *)take(b_members);
    a.member_chunk = (uint32_t *)take(b_m32);
    a.crcs = (uint32_t *)take(b_m32);
    a.chunks = (DfChunkDesc *)take(b_chunks);
    a.results = (DfResult *)take(b_res);
    a.chunk_off = (uint64_t *)take(b_coff);
    a.text = d_text;
    a.n = n;
    a.off = d_off;
    a.n_rec = n_rec;
    a.off_base = off_base;
    a.n_cells = C;
    a.tokens = (uint32_t *)d_tokens;
    a.stage = (uint8_t *)d_stage;
    a.out = d_out;
    a.workgroups = wgs;
    a.max_members = M;
    a.max_chunks = N;
    uint64_t got[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    launch_bgzf_plan(a, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(got, a.counts, 3 * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (got[0] > M || got[1] > N || got[1] < got[0] || got[2] != n)
        return set_err(ctx, NTC_ERR_INVALID_ARG, "BGZF plan: the record offsets do not describe the text");
    a.n_members = (uint32_t)got[0];
    a.n_chunks = (uint32_t)got[1];
    if (!a.n_members) return NTC_OK;
    launch_bgzf_code(a, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    const size_t t0 = tab.size();
    tab.resize(t0 + a.n_members);
    HIP_TRY(ctx, hipMemcpyAsync(tab.data() + t0, a.members, a.n_members * sizeof(BgzfMember), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(got, a.counts, 7 * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t i = t0; i < tab.size(); i++) tab[i].place += place_base;
    for (int i = 0; i < 7; i++) counts[i] += got[i];
    return NTC_OK;
}

// what both ntc_bgzf_compress calls refuse before anything runs (off on the host)
int bgzf_check(ntc_ctx *ctx, uint64_t n, const uint64_t *off, uint64_t n_rec, uint64_t out_cap, uint64_t *out_bytes) {
    if (off) {
        if (off[0] != 0 || off[n_rec] != n) return set_err(ctx, NTC_ERR_INVALID_ARG, "record offsets must start at 0 and end at n");
        for (uint64_t r = 0; r < n_rec; r++)
            if (off[r] > off[r + 1]) return set_err(ctx, NTC_ERR_INVALID_ARG, "record offsets decrease at record " + std::to_string(r));
    }
    *out_bytes = bgzf_bound(n);
    if (out_cap < bgzf_bound(n))
        return set_err(ctx, NTC_ERR_CAPACITY, "BGZF output needs " + std::to_string(bgzf_bound(n)) + " bytes");
    *out_bytes = 0;
    return NTC_OK;
}

// the table to the caller: NTC_ERR_CAPACITY (with *n_members set) when it does not fit
int bgzf_table_out(ntc_ctx *ctx, const std::vector<BgzfMember> &tab, ntc_bgzf_member *members, uint64_t members_cap, uint64_t *n_members) {
    *n_members = tab.size();
    if (!members) return NTC_OK;
    if (tab.size() > members_cap) return set_err(ctx, NTC_ERR_CAPACITY, "member array too small");
    if (!tab.empty()) std::memcpy(members, tab.data(), tab.size() * sizeof(BgzfMember));
    return NTC_OK;
}
}  // namespace

extern "C" {

uint64_t ntc_bgzf_bound(uint64_t n) { return bgzf_bound(n); }

int ntc_bgzf_compress(ntc_ctx *ctx, const uint8_t *text, uint64_t n, const uint64_t *rec_off, uint64_t n_rec, uint8_t *out,
                      uint64_t out_cap, ntc_bgzf_member *members, uint64_t members_cap, uint64_t *n_members, uint64_t *out_bytes) {
    if (!n_members || !out_bytes || (n && (!text || !out))) return set_err(ctx, NTC_ERR_INVALID_ARG, "null argument");
    *n_members = 0;
    int rc;
    if ((rc = bgzf_check(ctx, n, rec_off, n_rec, out_cap, out_bytes))) return rc;
    std::vector<BgzfMember> tab;
    uint64_t counts[7] = {0, 0, 0, 0, 0, 0, 0};
    if (!ctx) {
        bgzf_host(text, n, rec_off, n_rec, out, tab, counts);
        *out_bytes = counts[3];
        return bgzf_table_out(ctx, tab, members, members_cap, n_members);
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ctx->bz.begin();
    const auto t_bz = std::chrono::steady_clock::now();
    void *d_text, *d_off = nullptr, *d_out;
    if ((rc = ensure(ctx, WS_BZ_TEXT, n + 16, &d_text))) return rc;
    if ((rc = ensure(ctx, WS_BZ_OUT, bgzf_bound(n), &d_out))) return rc;
    if (rec_off && (rc = ensure(ctx, WS_BZ_OFF, (n_rec + 1) * 8, &d_off))) return rc;
    if (n) HIP_TRY(ctx, hipMemcpyAsync(d_text, text, n, hipMemcpyHostToDevice, ctx->stream));
    if (rec_off) HIP_TRY(ctx, hipMemcpyAsync(d_off, rec_off, (n_rec + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (the caller's buffers are pageable: nothing reads them after the return)
    if ((rc = bgzf_dev(ctx, (const uint8_t *)d_text, n, (const uint64_t *)d_off, n_rec, 0, (uint8_t *)d_out, 0, tab, counts))) return rc;
    if ((rc = bgzf_table_out(ctx, tab, members, members_cap, n_members))) return rc;
    if (counts[3]) HIP_TRY(ctx, hipMemcpy(out, d_out, counts[3], hipMemcpyDeviceToHost));
    *out_bytes = counts[3];
    std::copy(counts, counts + 7, ctx->bz.counts);
    ctx->bz.members = std::move(tab);
    ctx->bz.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_bz).count();
    return NTC_OK;
}

int ntc_bgzf_compress_device(ntc_ctx *ctx, const void *d_text, uint64_t n, const uint64_t *d_rec_off, uint64_t n_rec, void *d_out,
                             uint64_t out_cap, ntc_bgzf_member *members, uint64_t members_cap, uint64_t *n_members,
                             uint64_t *out_bytes) {
    if (!ctx || !n_members || !out_bytes || (n && (!d_text || !d_out))) return set_err(ctx, NTC_ERR_INVALID_ARG, "null argument");
    *n_members = 0;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc;
    std::vector<uint64_t> off;
    if (d_rec_off) {  // the offsets are checked on the host, as ntc_bgzf_compress checks them
        off.resize(n_rec + 1);
        HIP_TRY(ctx, hipMemcpyAsync(off.data(), d_rec_off, (n_rec + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    if ((rc = bgzf_check(ctx, n, d_rec_off ? off.data() : nullptr, n_rec, out_cap, out_bytes))) return rc;
    ctx->bz.begin();
    const auto t_bz = std::chrono::steady_clock::now();
    std::vector<BgzfMember> tab;
    uint64_t counts[7] = {0, 0, 0, 0, 0, 0, 0};
    if ((rc = bgzf_dev(ctx, (const uint8_t *)d_text, n, d_rec_off, n_rec, 0, (uint8_t *)d_out, 0, tab, counts))) return rc;
    if ((rc = bgzf_table_out(ctx, tab, members, members_cap, n_members))) return rc;
    *out_bytes = counts[3];
    std::copy(counts, counts + 7, ctx->bz.counts);
    ctx->bz.members = std::move(tab);
    ctx->bz.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_bz).count();
    return NTC_OK;
}

int ntc_bgzf_last(ntc_ctx *ctx, ntc_bgzf_counts *counts, ntc_bgzf_member *members, uint64_t members_cap, uint64_t *n_members) {
    if (!ctx || !counts || !n_members) return set_err(ctx, NTC_ERR_INVALID_ARG, "null argument");
    const uint64_t *c = ctx->bz.counts;
    *counts = ntc_bgzf_counts{c[0], c[2], c[3], c[4], c[5], c[6], ctx->bz.seconds};
    return bgzf_table_out(ctx, ctx->bz.members, members, members_cap, n_members);
}

}  // extern "C"

// The file pipeline's inflater (`--inflate gpu`, ntc_internal.h IHooks): one per encode call, on
// the first context's device, used by the reader thread alone.  It owns a stream, grow-only
// device buffers for a run's compressed bytes, descriptors, text and results, and a pinned
// staging buffer that takes the compressed bytes (the reader's window is pageable) and the
// results.  The text goes from the device straight to the caller's buffer.
namespace ntc {
struct Inflater {
    int device = 0;
    hipStream_t stream = nullptr;
    void *d_comp = nullptr, *d_text = nullptr, *d_desc = nullptr, *d_res = nullptr;
    uint64_t comp_cap = 0, text_cap = 0, n_cap = 0;
    uint8_t *stage = nullptr;  // pinned: compressed bytes, then descriptors, then results
    uint64_t stage_cap = 0;
    std::mutex mu;
    ~Inflater() {
        (void)hipSetDevice(device);
        for (void *p : {d_comp, d_text, d_desc, d_res})
            if (p) (void)hipFree(p);
        if (stage) (void)hipHostFree(stage);
        if (stream) (void)hipStreamDestroy(stream);
    }
    static bool grow(void **p, uint64_t *cap, uint64_t want) {
        if (*cap >= want) return true;
        if (*p) (void)hipFree(*p);
        *p = nullptr, *cap = 0;
        want += want / 4 + 4096;
        if (hipMalloc(p, want) != hipSuccess) return (void)hipGetLastError(), false;
        *cap = want;
        return true;
    }
    int run(const uint8_t *comp, uint64_t comp_bytes, const ntc_inflate_member *m, uint64_t n, uint8_t *dst, uint64_t dst_bytes,
            uint64_t *n_failed) {
        *n_failed = 0;
        if (!n) return NTC_OK;
        if (n >> 31) return NTC_ERR_CAPACITY;
        std::lock_guard<std::mutex> guard(mu);  // (a pair's two readers share it)
        // (the reader lays the members back to back in comp and dst: nothing to check but the ends)
        for (uint64_t i = 0; i < n; i++)
            if (m[i].src_off + m[i].src_bytes > comp_bytes || m[i].dst_off + m[i].out_bytes > dst_bytes ||
                (i && m[i].dst_off < m[i - 1].dst_off + m[i - 1].out_bytes))
                return NTC_ERR_INVALID_ARG;
        if (hipSetDevice(device) != hipSuccess) return NTC_ERR_HIP;
        const uint64_t desc_bytes = n * sizeof(InfMemberDesc), res_bytes = n * sizeof(InfResult);
        const uint64_t comp_room = (comp_bytes + 63) & ~63ull;
        const uint64_t need = comp_room + desc_bytes + res_bytes;
        if (stage_cap < need) {
            if (stage) (void)hipHostFree(stage);
            stage = nullptr, stage_cap = 0;
            if (hipHostMalloc((void **)&stage, need + need / 4, hipHostMallocDefault) != hipSuccess) return NTC_ERR_HIP;
            stage_cap = need + need / 4;
        }
        uint64_t cap_desc = n_cap * sizeof(InfMemberDesc), cap_res = n_cap * sizeof(InfResult);
        if (!grow(&d_comp, &comp_cap, comp_bytes) || !grow(&d_text, &text_cap, dst_bytes) || !grow(&d_desc, &cap_desc, desc_bytes) ||
            !grow(&d_res, &cap_res, res_bytes))
            return NTC_ERR_CAPACITY;
        n_cap = std::min(cap_desc / sizeof(InfMemberDesc), cap_res / sizeof(InfResult));
        std::memcpy(stage, comp, comp_bytes);
        InfMemberDesc *h_desc = (InfMemberDesc *)(stage + comp_room);
        for (uint64_t i = 0; i < n; i++) h_desc[i] = InfMemberDesc{m[i].src_off, m[i].src_bytes, m[i].out_bytes, m[i].dst_off};
        InfResult *h_res = (InfResult *)(stage + comp_room + desc_bytes);
        if (hipMemcpyAsync(d_comp, stage, comp_bytes, hipMemcpyHostToDevice, stream) != hipSuccess ||
            hipMemcpyAsync(d_desc, h_desc, desc_bytes, hipMemcpyHostToDevice, stream) != hipSuccess)
            return NTC_ERR_HIP;
        InfArgs a{};
        a.comp = (const uint8_t *)d_comp;
        a.members = (const InfMemberDesc *)d_desc;
        a.n_members = (uint32_t)n;
        a.dst = (uint8_t *)d_text;
        a.results = (InfResult *)d_res;
        launch_inflate(a, stream);
        if (hipGetLastError() != hipSuccess ||
            hipMemcpyAsync(h_res, d_res, res_bytes, hipMemcpyDeviceToHost, stream) != hipSuccess ||
            hipStreamSynchronize(stream) != hipSuccess)
            return NTC_ERR_HIP;
        for (uint64_t i = 0; i < n; i++) *n_failed += h_res[i].status != 0;
        if (*n_failed) return NTC_OK;  // nothing of the run is delivered
        if (dst_bytes && (hipMemcpyAsync(dst, d_text, dst_bytes, hipMemcpyDeviceToHost, stream) != hipSuccess ||
                          hipStreamSynchronize(stream) != hipSuccess))
            return NTC_ERR_HIP;
        return NTC_OK;
    }
};
}  // namespace ntc

namespace {
// encode + GPU block packer over reads already in HBM (d_offs: n_reads + 1 offsets, room for
// n_reads + 1 more behind them, where the record offsets go); the tail of
// ntc_encode_pack_batch and ntc_encode_pack_fastq.  dg: the digest components of the call (0:
// none); sym and seq are taken here, around the non-ACGT pass, and again (zeroed first) when
// the batch is staged afresh.  A re-run with grown pools encodes the same staged bases and
// leaves the digests alone.
int encode_pack_staged(ntc_ctx *ctx, const uint8_t *d_bases, const uint64_t *d_offs, uint64_t n_reads, uint64_t total,
                       uint32_t block_reads, ntc_block_meta *meta, uint8_t **payload, uint64_t *payload_bytes,
                       int64_t *bad_read, const std::function<int()> &restage, uint32_t dg) {
    void *d_recs, *d_payload;
    int rc;
    if ((rc = ensure(ctx, WS_STAGE_RECS, (total + 1) * 8, &d_recs))) return rc;
    uint64_t *d_roffs = (uint64_t *)d_offs + (n_reads + 1);
    // non-ACGT symbols are masked in the staged copy first (policy 0: nothing runs); a batch
    // with more runs than the list had room for is staged and run once more
    for (bool again = true; again;) {
        // (qual and name were taken from the text before this point, where the call has them)
        if (dg && (rc = dg_init(ctx, d_offs, n_reads, block_reads, dg, dg & (kDgQual | kDgName)))) return rc;
        if ((dg & kDgSym) && (rc = dg_add(ctx, 1, d_bases, total, d_offs, nullptr, nullptr, n_reads, block_reads))) return rc;
        if ((rc = nx_mask(ctx, const_cast<uint8_t *>(d_bases), d_offs, n_reads, total))) return rc;
        if (dg && (rc = dg_add(ctx, 0, d_bases, total, d_offs, nullptr, nullptr, n_reads, block_reads))) return rc;
        rc = encode4_impl(ctx, d_bases, d_offs, n_reads, total, (uint64_t *)d_recs, total + 1, d_roffs);
        if (rc) return rc;
        int64_t bad = -1;
        if ((rc = read_status(ctx, &bad))) {
            if (bad_read) *bad_read = bad;
            return rc;
        }
        if ((rc = nx_collect(ctx, 0, &again))) return rc;
        if (again && (rc = restage())) return rc;
    }
    // the payload never exceeds the records' 8 B each plus per-stream rounding, except for
    // malformed unary runs: size the device buffer for that and let the packer check
    const uint64_t n_blocks = (n_reads + block_reads - 1) / block_reads;
    uint64_t nrec = 0;  // the status box of the encode call holds it (k_emit4 wrote offsets from 0)
    if (ctx->box_valid) nrec = box(ctx, kBoxA);
    else HIP_TRY(ctx, hipMemcpy(&nrec, d_roffs + n_reads, 8, hipMemcpyDeviceToHost));
    const uint64_t ends[2] = {0, nrec};
    uint64_t cap = nrec * 10 + n_blocks * 64 + 64, used = 0;
    for (int attempt = 0;; attempt++) {
        if ((rc = ensure(ctx, WS_PACK_PAYLOAD, cap, &d_payload))) return rc;
        rc = pack_blocks_impl(ctx, (const uint64_t *)d_recs, d_roffs, n_reads, block_reads, (uint8_t *)d_payload,
                              ctx->ws[WS_PACK_PAYLOAD].bytes, meta, &used, ends);
        if (rc != NTC_ERR_CAPACITY || attempt) break;
        cap = used;  // exact requirement from the first pass
    }
    if (rc) return rc;
    if (ctx->df.opt) {  // option "gpu_deflate": the members in place of the raw streams, which stay in HBM
        uint64_t bound = 0;
        for (uint64_t b = 0; b < n_blocks; b++)
            for (int s = 0; s < 4 && meta[b].status == NTC_OK; s++) bound += df_member_bound(meta[b].stream[s].encoded_size * 8);
        void *d_members;
        if ((rc = ensure(ctx, WS_DF_OUT, bound, &d_members))) return rc;
        ctx->df.members.assign(n_blocks * 8, 0);
        if ((rc = deflate_blocks_impl(ctx, (const uint8_t *)d_payload, meta, n_blocks, (uint8_t *)d_members,
                                      ctx->ws[WS_DF_OUT].bytes, ctx->df.members.data(), &used))) {
            ctx->df.members.clear();
            return rc;
        }
        d_payload = d_members;
    }
    uint8_t *h = (uint8_t *)std::malloc(used ? used : 1);
    if (!h) return set_err(ctx, NTC_ERR_CAPACITY, "host payload allocation");
    if (used && hipMemcpy(h, d_payload, used, hipMemcpyDeviceToHost) != hipSuccess) {
        std::free(h);
        return set_err(ctx, NTC_ERR_HIP, "payload copy");
    }
    *payload = h;
    *payload_bytes = used;
    if (dg) ctx->dig.blocks = n_blocks;
    return NTC_OK;
}
}  // namespace

extern "C" {

int ntc_encode_pack_batch(ntc_ctx *ctx, const uint8_t *bases, const uint64_t *read_offsets, uint64_t n_reads,
                          uint32_t block_reads, ntc_block_meta *meta, uint8_t **payload, uint64_t *payload_bytes,
                          int64_t *bad_read) {
    if (bad_read) *bad_read = -1;
    if (!ctx || !read_offsets || !meta || !payload || !payload_bytes || block_reads == 0 || (n_reads && !bases))
        return set_err(ctx, NTC_ERR_INVALID_ARG, "null argument or block_reads = 0");
    *payload = nullptr;
    *payload_bytes = 0;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!ctx->has_index) return set_err(ctx, NTC_ERR_NO_INDEX, "no index uploaded");
    if (ctx->encode_variant != 4) return set_err(ctx, NTC_ERR_UNSUPPORTED, "encode_pack needs encode_variant 4");
    if (ctx->qual.mode != 0) return q_unsupported(ctx, "ntc_encode_pack_batch");
    if (ctx->names.mode != 0) return n_unsupported(ctx, "ntc_encode_pack_batch");
    ctx->dig.begin();
    ctx->df.begin();
    for (uint64_t r = 0; r < n_reads; r++)
        if (read_offsets[r + 1] < read_offsets[r])
            return set_err(ctx, NTC_ERR_INVALID_ARG, "read offsets must be non-decreasing");
    if (n_reads == 0) return NTC_OK;
    const uint64_t o0 = read_offsets[0], total = read_offsets[n_reads] - o0;
    std::vector<uint64_t> offs(n_reads + 1);
    for (uint64_t r = 0; r <= n_reads; r++) offs[r] = read_offsets[r] - o0;
    void *d_bases, *d_offs;
    int rc;
    if ((rc = ensure(ctx, WS_STAGE_BASES, total + 64, &d_bases))) return rc;
    if ((rc = ensure(ctx, WS_STAGE_OFFS, (n_reads + 1) * 8 * 2, &d_offs))) return rc;
    if (total) HIP_TRY(ctx, hipMemcpyAsync(d_bases, bases + o0, total, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d_offs, offs.data(), (n_reads + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    ctx->nx.begin();
    const auto restage = [&]() -> int {
        if (total) HIP_TRY(ctx, hipMemcpyAsync(d_bases, bases + o0, total, hipMemcpyHostToDevice, ctx->stream));
        return NTC_OK;
    };
    return encode_pack_staged(ctx, (const uint8_t *)d_bases, (const uint64_t *)d_offs, n_reads, total, block_reads,
                              meta, payload, payload_bytes, bad_read, restage, dg_components(ctx, false));
}

}  // extern "C"

namespace {
// FASTQ text -> bases (WS_STAGE_BASES) + read offsets (WS_STAGE_OFFS, room for the record
// offsets behind them) in HBM, parsed on the device (fastq.hip); synchronous, so the
// structure checks are answered before anything is encoded.  *total = bases kept.
//
// Pairs (option "paired", pairs.hip): with pair given, the text is woven on the device from the
// two mate texts (bytes = the woven size, fastq unused); with mate_check the names of reads 2p
// and 2p + 1 are compared after the parse.  Both verdicts arrive with the parse's own, at the
// one sync below.
struct PairSrc {
    const uint8_t *text[2];
    uint64_t bytes[2];
};

int pair_weave(ntc_ctx *ctx, const PairSrc &src, uint64_t n_pairs, uint8_t *d_raw, uint64_t woven, uint64_t *tmp,
               unsigned long long *status) {
    if (n_pairs == 0) return NTC_OK;
    const uint64_t at1 = (src.bytes[0] + 63) & ~63ull;  // (the line passes load 16 bytes at a time)
    const uint64_t tiles[2] = {fastq_tiles(src.bytes[0]), fastq_tiles(src.bytes[1])};
    void *in, *tab;
    int rc;
    if ((rc = ensure(ctx, WS_PAIR_IN, at1 + src.bytes[1] + 64, &in))) return rc;
    const uint64_t words = (tiles[0] + 1) + (tiles[1] + 1) + (n_pairs + 1);
    if ((rc = ensure(ctx, WS_PAIR_TAB, words * 8 + (tiles[0] + tiles[1] + 8 * n_pairs + n_pairs + 1) * 4 + 8, &tab)))
        return rc;
    PairWeaveArgs a{};
    uint64_t *w = (uint64_t *)tab;
    uint64_t *tile_base[2] = {w, w + tiles[0] + 1};
    a.offs = w + (tiles[0] + 1) + (tiles[1] + 1);
    uint32_t *h = (uint32_t *)(w + words);
    uint32_t *tile_cnt[2] = {h, h + tiles[0]};
    uint32_t *nl[2] = {h + tiles[0] + tiles[1], h + tiles[0] + tiles[1] + 4 * n_pairs};
    a.sizes = nl[1] + 4 * n_pairs;
    for (int t = 0; t < 2; t++) {
        uint8_t *d = (uint8_t *)in + (t ? at1 : 0);
        if (src.bytes[t]) HIP_TRY(ctx, hipMemcpyAsync(d, src.text[t], src.bytes[t], hipMemcpyHostToDevice, ctx->stream));
        launch_fastq_lines(d, src.bytes[t], tile_cnt[t], tile_base[t], nl[t], 4 * n_pairs, tmp, ctx->stream);
        a.raw[t] = d;
        a.n_raw[t] = src.bytes[t];
        a.nl[t] = nl[t];
        a.n_nl_p[t] = tile_base[t] + tiles[t];
    }
    a.n_pairs = n_pairs;
    a.tmp = tmp;
    a.out = d_raw;
    a.out_bytes = woven;
    a.status = status;
    launch_pair_weave(a, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    return NTC_OK;
}

int fastq_stage(ntc_ctx *ctx, const uint8_t *fastq, uint64_t bytes, uint64_t n_reads, void **d_bases, void **d_offs,
                uint64_t *total, int64_t *bad_read, const PairSrc *pair = nullptr, bool mate_check = false) {
    if (bad_read) *bad_read = -1;
    *total = 0;
    // The parse reuses d_status and the mailbox: whatever an earlier encode or decode
    // left there is gone, so its status / counts must not be reported any more.
    ctx->box_valid = false;
    ctx->last = kNone;
    if (bytes >= (1ull << 32)) return set_err(ctx, NTC_ERR_CAPACITY, "FASTQ text of 4 GiB or more: split the batch");
    if (n_reads == 0 && bytes) return set_err(ctx, NTC_ERR_FORMAT, "FASTQ text given for zero reads");
    const uint64_t tiles = fastq_tiles(bytes);
    void *raw, *tl, *nl, *kept, *tmp;
    int rc;
    if ((rc = ensure(ctx, WS_FQ_RAW, bytes + 64, &raw))) return rc;
    if ((rc = ensure(ctx, WS_FQ_TILES, tiles * 4 + (tiles + 1) * 8 + 8, &tl))) return rc;
    if ((rc = ensure(ctx, WS_FQ_NL, 4 * n_reads * 4 + 4, &nl))) return rc;
    if ((rc = ensure(ctx, WS_FQ_KEPT, n_reads * 4 + 4, &kept))) return rc;
    if ((rc = ensure(ctx, WS_SCANTMP, scan_tmp_words(std::max(tiles, n_reads) + 1) * 8, &tmp))) return rc;
    // a sequence line is no longer than its quality line, so bases <= bytes / 2
    if ((rc = ensure(ctx, WS_STAGE_BASES, bytes / 2 + 64, d_bases))) return rc;
    if ((rc = ensure(ctx, WS_STAGE_OFFS, (n_reads + 1) * 8 * 2, d_offs))) return rc;
    FastqArgs a{};
    a.raw = (const uint8_t *)raw;
    a.n_raw = bytes;
    a.n_reads = n_reads;
    a.tile_base = (uint64_t *)tl;
    a.tile_cnt = (uint32_t *)(a.tile_base + tiles + 1);
    a.nl = (uint32_t *)nl;
    a.kept = (uint32_t *)kept;
    a.offs = (uint64_t *)*d_offs;
    a.tmp = (uint64_t *)tmp;
    a.bases = (uint8_t *)*d_bases;
    a.status = ctx->d_status;
    unsigned long long *pst = nullptr;  // the weave's status word and the mate check's
    if (pair || mate_check) {
        void *p;
        if ((rc = ensure(ctx, WS_PAIR_ST, 64, &p))) return rc;
        pst = (unsigned long long *)p;
        HIP_TRY(ctx, hipMemsetAsync(pst, 0xFF, 16, ctx->stream));
        ctx->h_box[kBoxWeave] = ctx->h_box[kBoxMateCheck] = ~0ull;  // (no kernel of an earlier call writes them: each ends synchronised)
    }
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_status, 0xFF, 8, ctx->stream));
    if (pair) {
        if ((rc = pair_weave(ctx, *pair, n_reads / 2, (uint8_t *)raw, bytes, (uint64_t *)tmp, pst))) return rc;
    } else if (bytes) {
        HIP_TRY(ctx, hipMemcpyAsync(raw, fastq, bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    ctx->fq_last = a;
    launch_fastq_parse(a, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    if (pst) {
        if (mate_check) {
            PairCheckArgs c{};
            c.raw = a.raw;
            c.nl = a.nl;
            c.n_pairs = n_reads / 2;
            c.parse_status = ctx->d_status;
            c.status = pst + 1;
            launch_pair_check(c, ctx->stream);
        }
        launch_pair_box(pst, pst + 1, ctx->h_box, ctx->stream);
        HIP_TRY(ctx, hipGetLastError());
    }
    launch_status_box(ctx->d_status, a.offs + n_reads, nullptr, nullptr, ctx->h_box, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (pst && box(ctx, kBoxWeave) != ~0ULL) {  // (the parse then saw a text nobody wrote)
        const uint64_t w = box(ctx, kBoxWeave);
        if (bad_read) *bad_read = (int64_t)(w >> 8);
        char buf[160];
        std::snprintf(buf, sizeof(buf), "mate texts hold different record counts: read %lld has no whole record",
                      (long long)(w >> 8));
        return set_err(ctx, (int)(w & 0xFF), buf);
    }
    const uint64_t st = box(ctx, kBoxStatus);
    if (st != ~0ULL) {
        if (bad_read) *bad_read = (int64_t)(st >> 8);
        char buf[160];
        std::snprintf(buf, sizeof(buf), "malformed FASTQ record at index %lld", (long long)(st >> 8));
        return set_err(ctx, (int)(st & 0xFF), buf);
    }
    if (pst && box(ctx, kBoxMateCheck) != ~0ULL) {
        const uint64_t c = box(ctx, kBoxMateCheck);
        if (bad_read) *bad_read = (int64_t)(c >> 8);
        char buf[160];
        std::snprintf(buf, sizeof(buf), "the names of the mates disagree at pair %lld (reads %lld and %lld)",
                      (long long)(c >> 9), (long long)(c >> 8), (long long)(c >> 8) + 1);
        return set_err(ctx, (int)(c & 0xFF), buf);
    }
    *total = box(ctx, kBoxA);
    return NTC_OK;
}
}  // namespace

extern "C" {

int ntc_fastq_parse(ntc_ctx *ctx, const uint8_t *fastq, uint64_t fastq_bytes, uint64_t n_reads, uint8_t *bases_out,
                    uint64_t bases_capacity, uint64_t *read_offsets_out, uint64_t *n_bases, int64_t *bad_read) {
    if (bad_read) *bad_read = -1;
    if (!ctx || (fastq_bytes && !fastq) || !read_offsets_out) return set_err(ctx, NTC_ERR_INVALID_ARG, "null argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    void *d_bases, *d_offs;
    uint64_t total = 0;
    int rc = fastq_stage(ctx, fastq, fastq_bytes, n_reads, &d_bases, &d_offs, &total, bad_read);
    if (rc) return rc;
    if (n_bases) *n_bases = total;
    if (total > bases_capacity || (total && !bases_out))
        return set_err(ctx, NTC_ERR_CAPACITY, "bases_capacity smaller than the bases parsed");
    HIP_TRY(ctx, hipMemcpy(read_offsets_out, d_offs, (n_reads + 1) * 8, hipMemcpyDeviceToHost));
    if (total) HIP_TRY(ctx, hipMemcpy(bases_out, d_bases, total, hipMemcpyDeviceToHost));
    return NTC_OK;
}

}  // extern "C"

namespace {
// ntc_encode_pack_fastq, and ntc_encode_pack_fastq_paired (pair: the two texts to weave into
// the text of fastq_bytes bytes first)
int encode_pack_fastq_impl(ntc_ctx *ctx, const uint8_t *fastq, uint64_t fastq_bytes, uint64_t n_reads,
                           uint32_t block_reads, ntc_block_meta *meta, uint8_t **payload, uint64_t *payload_bytes,
                           uint64_t *n_bases, int64_t *bad_read, const PairSrc *pair) {
    *payload = nullptr;
    *payload_bytes = 0;
    if (n_bases) *n_bases = 0;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!ctx->has_index) return set_err(ctx, NTC_ERR_NO_INDEX, "no index uploaded");
    if (ctx->encode_variant != 4) return set_err(ctx, NTC_ERR_UNSUPPORTED, "encode_pack needs encode_variant 4");
    if (ctx->pair.mode && ((n_reads & 1) || (block_reads & 1)))
        return set_err(ctx, NTC_ERR_INVALID_ARG, "paired: n_reads and block_reads must be even");
    const bool smooth = ctx->qual.smooth != 0;
    if (smooth && ctx->qual.mode == 0)
        return set_err(ctx, NTC_ERR_INVALID_ARG, "quality_smooth needs qualities 1 (keep) or 2 (bin8)");
    if (smooth && qs_target((uint32_t)ctx->qual.mode, (uint32_t)ctx->qual.smooth_to) <= qs_floor((uint32_t)ctx->qual.mode))
        return set_err(ctx, NTC_ERR_INVALID_ARG, "quality_smooth_to: under bin8 the target's image must exceed that of '#'");
    void *d_bases, *d_offs;
    uint64_t total = 0;
    int rc = fastq_stage(ctx, fastq, fastq_bytes, n_reads, &d_bases, &d_offs, &total, bad_read, pair,
                         ctx->pair.mode == kPairIds);
    if (rc && ctx->pair.mode) side_begin(ctx);  // a failed call leaves no sections
    if (rc) return rc;
    if (n_bases) *n_bases = total;
    side_begin(ctx);
    if (n_reads == 0) return NTC_OK;
    // the digest table of the call (option "digests" 0: nothing runs here or below)
    const uint32_t dg = dg_components(ctx, true);
    if (dg && (rc = dg_init(ctx, (const uint64_t *)d_offs, n_reads, block_reads, dg, 0))) return rc;
    // the quality lines are packed from the text while the reads are encoded (mode 0: nothing runs)
    // (smoothing: only the gather; the rest and the qual digest follow the encode, q_finish below)
    if ((rc = q_pack(ctx, (const uint64_t *)d_offs, n_reads, total, block_reads, smooth))) return rc;
    if (!smooth && (dg & kDgQual) && (rc = dg_add(ctx, 2, ctx->ws[WS_Q_QUALS].p, total, (const uint64_t *)d_offs, nullptr, nullptr,
                                      n_reads, block_reads)))
        return rc;
    // and the names are front-coded from it (mode 0: nothing runs)
    if ((rc = n_pack(ctx, n_reads, block_reads))) return rc;
    if ((dg & kDgName) && (rc = dg_add(ctx, 3, ctx->fq_last.raw, ctx->fq_last.n_raw, nullptr, ctx->names.d_start, ctx->names.d_len,
                                      n_reads, block_reads)))
        return rc;
    const auto restage = [&]() -> int {  // the text is still in HBM: parse it again (it parsed clean once)
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_status, 0xFF, 8, ctx->stream));
        ctx->fq_last.tmp = (uint64_t *)ctx->ws[WS_SCANTMP].p;  // the scan scratch may have grown (never shrinks) since
        launch_fastq_parse(ctx->fq_last, ctx->stream);
        HIP_TRY(ctx, hipGetLastError());
        return NTC_OK;
    };
    rc = encode_pack_staged(ctx, (const uint8_t *)d_bases, (const uint64_t *)d_offs, n_reads, total, block_reads, meta,
                            payload, payload_bytes, bad_read, restage, dg);
    if (smooth) {
        if (rc) (void)hipStreamSynchronize(ctx->stream);  // (as below)
        const int frc = q_finish(ctx, rc == NTC_OK, (const uint64_t *)d_offs, n_reads, total, block_reads, dg);
        if (frc && !rc) {
            std::free(*payload);
            *payload = nullptr;
            *payload_bytes = 0;
            rc = frc;
        }
    }
    if (ctx->qual.mode == 0 && ctx->names.mode == 0) return rc;
    // a read the quality or the names pass refused fails the call, whatever the encode said of it
    if (rc) (void)hipStreamSynchronize(ctx->stream);  // (an encode that failed early may not have synchronised)
    int64_t q_bad = -1, n_bad = -1;
    const int qrc = q_collect(ctx, n_reads, block_reads, &q_bad);
    const int nrc = n_collect(ctx, n_reads, block_reads, &n_bad);
    const int src = qrc ? qrc : nrc;
    if (rc || src) {  // a failed call leaves no sections
        ctx->qual.begin();
        ctx->names.begin();
        ctx->dig.begin();
        ctx->df.begin();
    }
    if (src && bad_read) *bad_read = qrc ? q_bad : n_bad;
    if (src && !rc) {
        std::free(*payload);
        *payload = nullptr;
        *payload_bytes = 0;
    }
    return src ? src : rc;
}
}  // namespace

extern "C" {

int ntc_encode_pack_fastq(ntc_ctx *ctx, const uint8_t *fastq, uint64_t fastq_bytes, uint64_t n_reads,
                          uint32_t block_reads, ntc_block_meta *meta, uint8_t **payload, uint64_t *payload_bytes,
                          uint64_t *n_bases, int64_t *bad_read) {
    if (bad_read) *bad_read = -1;
    if (!ctx || (fastq_bytes && !fastq) || !meta || !payload || !payload_bytes || block_reads == 0)
        return set_err(ctx, NTC_ERR_INVALID_ARG, "null argument or block_reads = 0");
    return encode_pack_fastq_impl(ctx, fastq, fastq_bytes, n_reads, block_reads, meta, payload, payload_bytes, n_bases,
                                  bad_read, nullptr);
}

int ntc_encode_pack_fastq_paired(ntc_ctx *ctx, const uint8_t *fastq1, uint64_t bytes1, const uint8_t *fastq2,
                                 uint64_t bytes2, uint64_t n_pairs, uint32_t block_reads, ntc_block_meta *meta,
                                 uint8_t **payload, uint64_t *payload_bytes, uint64_t *n_bases, int64_t *bad_read) {
    if (bad_read) *bad_read = -1;
    if (!ctx || (bytes1 && !fastq1) || (bytes2 && !fastq2) || !meta || !payload || !payload_bytes || block_reads == 0)
        return set_err(ctx, NTC_ERR_INVALID_ARG, "null argument or block_reads = 0");
    *payload = nullptr;
    *payload_bytes = 0;
    if (n_bases) *n_bases = 0;
    if (!ctx->pair.mode) return set_err(ctx, NTC_ERR_INVALID_ARG, "ntc_encode_pack_fastq_paired needs the option paired 1 or 2");
    side_begin(ctx);  // a failed call leaves no sections
    // (the weave may add a newline to each text)
    if (bytes1 >= (1ull << 32) || bytes2 >= (1ull << 32) || bytes1 + bytes2 + 2 >= (1ull << 32))
        return set_err(ctx, NTC_ERR_CAPACITY, "mate texts of 4 GiB or more together: split the batch");
    // a record is four lines: a count no text under 4 GiB can hold fails before it sizes a table
    if (n_pairs > (1ull << 30) || (n_pairs == 0 && (bytes1 || bytes2)))
        return set_err(ctx, NTC_ERR_FORMAT, "mate texts hold different record counts: text given for zero pairs, or too many pairs");
    const PairSrc src{{fastq1, fastq2}, {bytes1, bytes2}};
    const uint64_t woven = bytes1 + bytes2 + (bytes1 && fastq1[bytes1 - 1] != '\n') + (bytes2 && fastq2[bytes2 - 1] != '\n');
    return encode_pack_fastq_impl(ctx, nullptr, woven, 2 * n_pairs, block_reads, meta, payload, payload_bytes, n_bases,
                                  bad_read, &src);
}

}  // extern "C"

namespace {
// bytes of ">seq.{id}\n" + read + "\n" for ids first_id .. first_id + n_reads - 1
uint64_t fasta_bytes(uint64_t n_reads, uint64_t n_bases, uint64_t first_id) {
    uint64_t need = n_bases + 7 * n_reads;  // 5 + 2 per read, plus the digits
    for (uint64_t lo = 1, d = 1; lo <= first_id + n_reads - 1 && n_reads; lo *= 10, d++) {
        const uint64_t hi = lo > UINT64_MAX / 10 ? UINT64_MAX : lo * 10 - 1;  // ids with d digits: [lo, hi]
        const uint64_t a = std::max(lo, first_id), b = std::min(hi, first_id + n_reads - 1);
        if (a <= b) need += d * (b - a + 1);
        if (hi == UINT64_MAX) break;
    }
    return need;
}

// the text a decode call writes: FASTQ when quality sections are pending ("\n+\n" and the
// qualities more per read)
uint64_t text_bytes(const ntc_ctx *ctx, uint64_t n_reads, uint64_t n_bases, uint64_t first_id) {
    const uint64_t q = ctx->qual.pending.has ? n_bases + 3 * n_reads : 0;
    // with names pending: ">" or "@", the name, '\n', the read, '\n' (and no seq.N)
    if (!ctx->names.pending.has) return fasta_bytes(n_reads, n_bases, first_id) + q;
    uint64_t name_bytes = 0;
    for (const ntc_name_meta &m : ctx->names.pending.metas) name_bytes += m.name_bytes;
    return name_bytes + n_bases + 3 * n_reads + q;
}

// The pending text window leaves the context with the call that takes it: a size query (keep)
// alone leaves it for the call it sizes.
struct TextWindow {
    ntc_ctx *ctx;
    uint64_t first = 0, count = 0;  // count 0: no window
    bool kept = false;
    explicit TextWindow(ntc_ctx *c) : ctx(c) {
        if (c->win.has_pending) first = c->win.first, count = c->win.count;
    }
    ~TextWindow() {
        if (!kept) ctx->win.has_pending = false;
    }
    void keep() { kept = true; }
    // the request against the batch it met
    int check(uint64_t n_reads) const {
        if (!count || w_valid(first, count, n_reads, ctx->pair.mode != 0)) return NTC_OK;
        const bool inside = first < n_reads && count <= n_reads - first;  // (then it cuts a pair)
        return set_err(ctx, NTC_ERR_INVALID_ARG, inside ? "paired: a window's first read and count must be even (whole pairs)"
                                                        : "the window reaches past the batch's reads");
    }
};

// the sections of a side stream taken for this call cover exactly the reads it decodes
template <class Meta>
int sections_cover(ntc_ctx *ctx, const std::vector<Meta> &metas, uint64_t n_reads, const char *noun) {
    uint64_t r = 0;
    for (const Meta &m : metas) {
        if (m.n_reads > n_reads - r)
            return set_err(ctx, NTC_ERR_FORMAT, std::string(noun) + " sections for more reads than decoded");
        r += m.n_reads;
    }
    if (r != n_reads) return set_err(ctx, NTC_ERR_FORMAT, std::string(noun) + " sections for fewer reads than decoded");
    return NTC_OK;
}

// option "bgzf_text": the room a text of `need` bytes asks of the caller's buffer (two parts under
// the pair split: each may round its member count up once more)
uint64_t bgzf_text_room(uint64_t need) { return bgzf_bound(need) + 2 * (uint64_t)kBgzfSlack; }

// walk + FASTA text of records already in HBM (d_recs), text D2H into out (need bytes; with a
// window w only the window's bytes, which *out_len then reports)
int decode_fasta_dev(ntc_ctx *ctx, const uint64_t *d_recs, uint64_t n_recs, uint64_t n_reads, uint64_t n_bases,
                     uint64_t first_id, uint8_t *out, uint64_t need, const TextWindow &w, uint64_t *out_len) {
    void *d_bases, *d_offs, *d_scan, *d_out;
    int rc;
    if ((rc = ensure(ctx, WS_FA_BASES, n_bases + 64, &d_bases))) return rc;
    if ((rc = ensure(ctx, WS_FA_OFFS, (n_reads + 2) * 8, &d_offs))) return rc;
    if ((rc = ensure(ctx, WS_FA_SCAN, (2 * (n_reads + 1) + scan_tmp_words(n_reads + 1)) * 8, &d_scan))) return rc;
    if ((rc = ensure(ctx, WS_STAGE_BASES, need + 64, &d_out))) return rc;
    // pairs: the formatted text is split into its two parts on the device before the copy
    const bool split = ctx->pair.mode && !ctx->discard_text && n_reads;
    void *d_pscan = nullptr, *d_split = nullptr;
    if (split) {
        if ((rc = ensure(ctx, WS_PAIR_SCAN, 4 * (n_reads / 2 + 1) * 8, &d_pscan))) return rc;
        if ((rc = ensure(ctx, WS_PAIR_OUT, need + 64, &d_split))) return rc;
    }
    Pending<ntc_nx_run> nxp;
    Pending<ntc_qual_meta> qs;
    Pending<ntc_name_meta> ns;
    Pending<ntc_digest_meta> ds;
    const bool fastq = ctx->qual.pending.take(qs);  // (all pending lists leave the context here)
    const bool named = ctx->names.pending.take(ns);
    const bool digests = ctx->dig.pending.take(ds);
    const bool has_nx = ctx->nx.pending.take(nxp);
    const std::vector<ntc_nx_run> &nx = nxp.metas;
    const uint32_t nx_sub = ctx->nx.pending_sub;
    if ((rc = w.check(n_reads))) return rc;  // (after the lists: a refused window leaves nothing pending either)
    if (has_nx && nx.back().read >= n_reads)
        return set_err(ctx, NTC_ERR_FORMAT, "exception run past the last read");
    if (fastq && (rc = sections_cover(ctx, qs.metas, n_reads, "quality"))) return rc;
    if (named && (rc = sections_cover(ctx, ns.metas, n_reads, "name"))) return rc;
    DgDecode dg;
    if (digests && (rc = sections_cover(ctx, ds.metas, n_reads, "digest"))) return rc;
    if (digests && (rc = dgd_begin(ctx, ds.metas, dg))) return rc;
    if ((rc = ntc_decode_batch_device(ctx, d_recs, n_recs, (uint8_t *)d_bases, n_bases + 64, (uint64_t *)d_offs,
                                      n_reads + 2)))
        return rc;
    // the walked bases are digested as they stand (seq), before the exception runs go in
    if (digests && (rc = dgd_add(ctx, dg, 0, d_bases, n_bases, (const uint64_t *)d_offs))) return rc;
    // exception runs go over the substitute bases before the text is formatted
    if (!nx.empty() && (rc = nx_patch(ctx, nx, nx_sub, 0, n_reads, (uint8_t *)d_bases, (const uint64_t *)d_offs)))
        return rc;
    // (sym: only then is there anything to tell from seq)
    if (digests && !nx.empty() && (rc = dgd_add(ctx, dg, 1, d_bases, n_bases, (const uint64_t *)d_offs))) return rc;
    // and the qualities are unpacked by the decoded reads' offsets, after the patch
    uint8_t *d_quals = nullptr;
    if (fastq && (rc = q_unpack(ctx, qs.metas, qs.payload, n_reads, n_bases, (const uint64_t *)d_offs, &d_quals))) return rc;
    // and the names are expanded, each section on its own
    uint8_t *d_names = nullptr;
    uint64_t *d_name_off = nullptr;
    if (named && (rc = n_expand(ctx, ns.metas, ns.payload, n_reads, &d_names, &d_name_off))) return rc;
    // the other two components over what was just expanded, then the verdict on the device:
    // a block that differs sets the status, and the formatters below write nothing
    if (digests) {
        uint64_t name_bytes = 0;
        for (const ntc_name_meta &m : ns.metas) name_bytes += m.name_bytes;
        if (fastq && (rc = dgd_add(ctx, dg, 2, d_quals, n_bases, (const uint64_t *)d_offs))) return rc;
        if (named && (rc = dgd_add(ctx, dg, 3, d_names, name_bytes, d_name_off))) return rc;
        if ((rc = dgd_compare(ctx, dg, n_reads, (const uint64_t *)d_offs))) return rc;
    }
    uint64_t *sizes = (uint64_t *)d_scan, *out_offs = sizes + (n_reads + 1), *tmp = out_offs + (n_reads + 1);
    if (named)
        launch_named_text((const uint8_t *)d_bases, d_quals, (const uint64_t *)d_offs, d_names, d_name_off, n_reads,
                          ctx->d_status, sizes, out_offs, tmp, (uint8_t *)d_out, need, ctx->stream, w.first, w.count);
    else if (fastq)
        launch_fastq_text((const uint8_t *)d_bases, d_quals, (const uint64_t *)d_offs, n_reads, first_id, ctx->d_status,
                          sizes, out_offs, tmp, (uint8_t *)d_out, need, ctx->stream, w.first, w.count);
    else
        launch_fasta((const uint8_t *)d_bases, (const uint64_t *)d_offs, n_reads, first_id, ctx->d_status, sizes,
                     out_offs, tmp, (uint8_t *)d_out, need, ctx->stream, w.first, w.count);
    HIP_TRY(ctx, hipGetLastError());
    if (w.count) {  // the window's bytes: the scan's total, 0 when the call failed on the device
        ctx->h_box[kBoxWindow] = 0;  // (no kernel of an earlier call writes it: each ends synchronised)
        launch_window_box(out_offs + n_reads, ctx->h_box, ctx->stream);
        HIP_TRY(ctx, hipGetLastError());
    }
    if (split) {
        PairSplitArgs p{};
        p.text = (const uint8_t *)d_out;
        p.out_offs = out_offs;
        p.n_pairs = n_reads / 2;
        p.cap = need;
        p.s1 = (uint64_t *)d_pscan;
        p.s2 = p.s1 + (p.n_pairs + 1);
        p.o1 = p.s2 + (p.n_pairs + 1);
        p.o2 = p.o1 + (p.n_pairs + 1);
        p.tmp = tmp;  // (the formatter's scan is done with it)
        p.out = (uint8_t *)d_split;
        p.box = ctx->h_box;
        launch_pair_split(p, ctx->stream);
        HIP_TRY(ctx, hipGetLastError());
        d_out = d_split;
    }
    uint64_t copy = need;
    if (w.count) {  // the device knows the window's bytes: wait for them, copy only them
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        const uint64_t got = box(ctx, kBoxWindow);
        *out_len = copy = std::min(need, got);
    }
    // option "bgzf_text": the text stays on the device, its members are copied in its place below
    const bool bz = ctx->bz.opt && !ctx->discard_text;
    if (!ctx->discard_text && !bz && copy) HIP_TRY(ctx, hipMemcpyAsync(out, d_out, copy, hipMemcpyDeviceToHost, ctx->stream));
    uint64_t nr = 0, nb = 0;
    rc = ntc_decode_status(ctx, &nr, &nb);  // synchronises
    if (digests) rc = dgd_verdict(ctx, rc);
    if (rc) return rc;
    if (nr != n_reads || nb != n_bases)
        return set_err(ctx, NTC_ERR_FORMAT, "records hold other read / base counts than given");
    if (split) ctx->pair.first = box(ctx, kBoxPairFirst);
    if (bz) {  // the status is clear, so the text and its offsets stand: plan and code it, each part on its own
        BgzfState &B = ctx->bz;
        const auto t_bz = std::chrono::steady_clock::now();
        void *d_bz;
        if ((rc = ensure(ctx, WS_BZ_OUT, bgzf_text_room(copy), &d_bz))) return rc;
        const uint8_t *text = (const uint8_t *)d_out;
        if (split) {
            const uint64_t np = n_reads / 2, first = std::min(ctx->pair.first, copy);
            const uint64_t *o1 = (const uint64_t *)d_pscan + 2 * (np + 1), *o2 = o1 + (np + 1);
            if ((rc = bgzf_dev(ctx, text, first, o1, np, 0, (uint8_t *)d_bz, 0, B.members, B.counts))) return rc;
            const uint64_t part1 = B.counts[3];
            if ((rc = bgzf_dev(ctx, text + first, copy - first, o2, np, 0, (uint8_t *)d_bz + part1, part1, B.members, B.counts)))
                return rc;
            ctx->pair.first = part1;
        } else if ((rc = bgzf_dev(ctx, text, copy, out_offs, n_reads, 0, (uint8_t *)d_bz, 0, B.members, B.counts)))
            return rc;
        if (B.counts[3]) HIP_TRY(ctx, hipMemcpy(out, d_bz, B.counts[3], hipMemcpyDeviceToHost));
        *out_len = B.counts[3];
        B.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_bz).count();
    }
    return NTC_OK;
}
}  // namespace

namespace ntc {
int reserve_decode(ntc_ctx *ctx, uint64_t pay_bytes, uint64_t n_recs, uint8_t *host, uint64_t host_bytes) {
    if (!ctx) return NTC_ERR_INVALID_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint64_t pw = (pay_bytes + 7) / 8, n_bases = 40 * n_recs, need = fasta_bytes(n_recs, n_bases, 1);
    void *p;
    int rc;
    if ((rc = ensure(ctx, WS_UNP_PAY, pw * 8 + 16, &p))) return rc;
    if ((rc = ensure(ctx, WS_UNP_MARKS, pw * 8 * 8 + 128, &p))) return rc;  // marks + tile tables
    if ((rc = ensure(ctx, WS_UNP_VALS, 3 * n_recs * 8 + 8, &p))) return rc;
    if ((rc = ensure(ctx, WS_UNP_RECS, n_recs * 8 + 8, &p))) return rc;
    if ((rc = ensure(ctx, WS_FA_BASES, n_bases + 64, &p))) return rc;
    if ((rc = ensure(ctx, WS_FA_OFFS, (n_recs + 2) * 8, &p))) return rc;
    if ((rc = ensure(ctx, WS_FA_SCAN, (2 * (n_recs + 1) + scan_tmp_words(n_recs + 1)) * 8, &p))) return rc;
    if ((rc = ensure(ctx, WS_STAGE_BASES, need + 64, &p))) return rc;
    const uint64_t nc = std::min<uint64_t>({host_bytes, need + 64, 4u << 20});
    if (host && nc) {
        HIP_TRY(ctx, hipMemcpyAsync(host, p, nc, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(p, host, nc, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    return NTC_OK;
}
}  // namespace ntc

extern "C" {

int ntc_decode_fasta(ntc_ctx *ctx, const uint64_t *recs, uint64_t n_recs, uint64_t n_reads, uint64_t n_bases,
                     uint64_t first_id, uint8_t *out, uint64_t out_capacity, uint64_t *out_len) {
    if (!ctx || !out_len || (n_recs && !recs) || (n_reads && !out && !ctx->discard_text))
        return set_err(ctx, NTC_ERR_INVALID_ARG, "null argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    *out_len = 0;
    ctx->pair.valid = false;
    TextWindow w(ctx);
    if (!ctx->has_index) return set_err(ctx, NTC_ERR_NO_INDEX, "no index uploaded");
    if (ctx->pair.mode && (n_reads & 1)) return set_err(ctx, NTC_ERR_FORMAT, "paired: an odd number of reads");
    const uint64_t need = text_bytes(ctx, n_reads, n_bases, first_id);
    const bool bz = ctx->bz.opt && !ctx->discard_text;
    if (ctx->bz.opt) ctx->bz.begin();
    *out_len = bz ? bgzf_text_room(need) : need;
    if (*out_len > out_capacity && !ctx->discard_text) {
        w.keep();  // (a size query: the window waits for the call it sizes)
        return set_err(ctx, NTC_ERR_CAPACITY, bz ? "out_capacity smaller than the bound of the text's BGZF members"
                                                 : "out_capacity smaller than the FASTA text");
    }
    ctx->pair.valid = ctx->pair.mode && !ctx->discard_text;  // (the parts stay empty unless the call succeeds)
    ctx->pair.first = 0;
    if (n_recs == 0) {
        if (bz) *out_len = 0;
        if (const int wrc = w.check(n_reads)) return wrc;
        return n_reads ? set_err(ctx, NTC_ERR_FORMAT, "reads without records") : NTC_OK;
    }
    void *d_recs;
    int rc;
    if ((rc = ensure(ctx, WS_STAGE_RECS, n_recs * 8, &d_recs))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(d_recs, recs, n_recs * 8, hipMemcpyHostToDevice, ctx->stream));
    return decode_fasta_dev(ctx, (const uint64_t *)d_recs, n_recs, n_reads, n_bases, first_id, out, need, w, out_len);
}

int ntc_unpack_streams(ntc_ctx *ctx, const uint8_t *payload, uint64_t payload_bytes, const ntc_block_meta *metas,
                       uint64_t n_blocks, uint64_t *n_blocks_ok, uint64_t *n_reads, uint64_t *n_bases) {
    if (!ctx || (n_blocks && (!metas || !payload)) || !n_blocks_ok) return set_err(ctx, NTC_ERR_INVALID_ARG, "null argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    *n_blocks_ok = 0;
    if (n_reads) *n_reads = 0;
    if (n_bases) *n_bases = 0;
    ctx->unp_recs = 0;
    ctx->unp_reads = ctx->unp_bases = 0;
    ctx->unp_path[0] = ctx->unp_path[1] = ctx->unp_path[2] = 0;
    if (n_blocks == 0) return NTC_OK;
    // stream descriptors: word offsets into the payload, value offsets, record offsets
    std::vector<UnpackStream> st(4 * n_blocks);
    std::vector<uint64_t> roff(n_blocks + 1, 0);
    uint64_t nv = 0;
    const uint64_t pay_words = (payload_bytes + 7) / 8;
    for (uint64_t b = 0; b < n_blocks; b++) {
        for (int i = 0; i < 4; i++) {
            const ntc_stream_meta &m = metas[b].stream[i];
            if ((m.offset & 7) || m.offset / 8 + m.encoded_size > pay_words)
                return set_err(ctx, NTC_ERR_INVALID_ARG, "stream outside the payload or not 8-byte aligned");
            st[4 * b + i] = UnpackStream{m.offset / 8, m.encoded_size, m.num_u64, m.param, nv};
            nv += m.num_u64;
        }
        roff[b + 1] = roff[b] + metas[b].stream[2].num_u64;  // one flag per record
    }
    void *d_pay, *d_marks, *d_st, *d_vals, *d_recs, *d_out;
    int rc;
    if ((rc = ensure(ctx, WS_UNP_PAY, pay_words * 8 + 16, &d_pay))) return rc;
    // the tiles of the streams (their tables after the marks)
    UnpackPlan plan;
    unpack_plan(st.data(), n_blocks, plan);
    if ((rc = ensure(ctx, WS_UNP_MARKS, pay_words * 8 + 128 + unpack_ws_bytes(plan), &d_marks))) return rc;
    void *d_ws = (uint8_t *)d_marks + ((pay_words * 8 + 16 + 63) & ~63ull);
    // the table upload: streams, record offsets, tile lists, stream lists
    const std::vector<UnpTile> *tl[2] = {&plan.mb_tiles, &plan.rice_tiles};
    const std::vector<UnpStreamRef> *sl[2] = {&plan.mb_streams, &plan.rice_streams};
    uint64_t up_bytes = st.size() * sizeof(UnpackStream) + (n_blocks + 1) * 8;
    for (int k = 0; k < 2; k++) up_bytes += tl[k]->size() * sizeof(UnpTile) + sl[k]->size() * sizeof(UnpStreamRef);
    std::vector<uint8_t> up(up_bytes);
    uint64_t at[4];
    {
        uint64_t q = 0;
        std::memcpy(up.data(), st.data(), st.size() * sizeof(UnpackStream));
        q += st.size() * sizeof(UnpackStream);
        std::memcpy(up.data() + q, roff.data(), (n_blocks + 1) * 8);
        q += (n_blocks + 1) * 8;
        for (int k = 0; k < 2; k++) {
            at[2 * k] = q;
            if (!tl[k]->empty()) std::memcpy(up.data() + q, tl[k]->data(), tl[k]->size() * sizeof(UnpTile));
            q += tl[k]->size() * sizeof(UnpTile);
            at[2 * k + 1] = q;
            if (!sl[k]->empty()) std::memcpy(up.data() + q, sl[k]->data(), sl[k]->size() * sizeof(UnpStreamRef));
            q += sl[k]->size() * sizeof(UnpStreamRef);
        }
    }
    if ((rc = ensure(ctx, WS_UNP_ST, up.size(), &d_st))) return rc;
    if ((rc = ensure(ctx, WS_UNP_VALS, nv * 8 + 8, &d_vals))) return rc;
    if ((rc = ensure(ctx, WS_UNP_RECS, roff[n_blocks] * 8 + 8, &d_recs))) return rc;
    uint64_t max_recs = 0;
    for (uint64_t b = 0; b < n_blocks; b++) max_recs = std::max<uint64_t>(max_recs, metas[b].stream[2].num_u64);
    const uint64_t segw = unpack_seg_words(n_blocks, max_recs);
    if ((rc = ensure(ctx, WS_UNP_OUT, (n_blocks * 3 + 3) * 8 + segw * 8 + 4 * n_blocks * 4 + 8, &d_out))) return rc;
    uint64_t *d_roff = (uint64_t *)((uint8_t *)d_st + st.size() * sizeof(UnpackStream));
    uint64_t *d_out3 = (uint64_t *)d_out, *d_segc = d_out3 + 3 * n_blocks + 3;  // (the path words between)
    int32_t *d_sst = (int32_t *)(d_segc + segw);
    HIP_TRY(ctx, hipMemcpyAsync(d_pay, payload, payload_bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d_st, up.data(), up.size(), hipMemcpyHostToDevice, ctx->stream));
    UnpackDev dv{};
    dv.payload = (const uint64_t *)d_pay;
    dv.st = (const UnpackStream *)d_st;
    dv.n_blocks = n_blocks;
    dv.max_recs = max_recs;
    dv.marks = (uint64_t *)d_marks;
    dv.mb_tiles = (const UnpTile *)((uint8_t *)d_st + at[0]);
    dv.mb_streams = (const UnpStreamRef *)((uint8_t *)d_st + at[1]);
    dv.rice_tiles = (const UnpTile *)((uint8_t *)d_st + at[2]);
    dv.rice_streams = (const UnpStreamRef *)((uint8_t *)d_st + at[3]);
    dv.n_mb_tiles = (uint32_t)plan.mb_tiles.size();
    dv.n_rice_tiles = (uint32_t)plan.rice_tiles.size();
    dv.n_mb_streams = (uint32_t)plan.mb_streams.size();
    dv.n_rice_streams = (uint32_t)plan.rice_streams.size();
    dv.ws = d_ws;
    dv.vals = (uint64_t *)d_vals;
    dv.status = d_sst;
    dv.rec_off = d_roff;
    dv.recs = (uint64_t *)d_recs;
    dv.segc = d_segc;
    dv.out3 = d_out3;
    launch_unpack(dv, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    std::vector<uint64_t> o3(3 * n_blocks + 3);  // out3 and the path words after it, in one copy
    HIP_TRY(ctx, hipMemcpyAsync(o3.data(), d_out3, (3 * n_blocks + 3) * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < 3; i++) ctx->unp_path[i] = o3[3 * n_blocks + i];
    // the blocks before the first damaged one (decode_block's Err ends the reference's loop,
    // main.rs:202); a block the host already found damaged (meta status) ends it as well
    uint64_t ok = 0, rd = 0, bs = 0;
    for (; ok < n_blocks && o3[3 * ok + 2] == 0 && metas[ok].status == 0; ok++) {
        rd += o3[3 * ok];
        bs += o3[3 * ok + 1];
    }
    *n_blocks_ok = ok;
    if (n_reads) *n_reads = rd;
    if (n_bases) *n_bases = bs;
    ctx->unp_d_recs = (uint64_t *)d_recs;
    ctx->unp_recs = roff[ok];
    ctx->unp_reads = rd;
    ctx->unp_bases = bs;
    return NTC_OK;
}

int ntc_unpacked_records(ntc_ctx *ctx, uint64_t *recs, uint64_t capacity, uint64_t *n_recs) {
    if (!ctx || !n_recs || (capacity && !recs)) return set_err(ctx, NTC_ERR_INVALID_ARG, "null argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    *n_recs = ctx->unp_recs;
    if (ctx->unp_recs > capacity) return set_err(ctx, NTC_ERR_CAPACITY, "capacity smaller than the unpacked records");
    if (ctx->unp_recs)
        HIP_TRY(ctx, hipMemcpy(recs, ctx->unp_d_recs, ctx->unp_recs * 8, hipMemcpyDeviceToHost));
    return NTC_OK;
}

int ntc_decode_fasta_unpacked(ntc_ctx *ctx, uint64_t first_id, uint8_t *out, uint64_t out_capacity, uint64_t *out_len) {
    if (!ctx || !out_len) return set_err(ctx, NTC_ERR_INVALID_ARG, "null argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    *out_len = 0;
    ctx->pair.valid = false;
    TextWindow w(ctx);
    if (!ctx->has_index) return set_err(ctx, NTC_ERR_NO_INDEX, "no index uploaded");
    if (ctx->pair.mode && (ctx->unp_reads & 1)) return set_err(ctx, NTC_ERR_FORMAT, "paired: an odd number of reads");
    const uint64_t need = text_bytes(ctx, ctx->unp_reads, ctx->unp_bases, first_id);
    const bool bz = ctx->bz.opt && !ctx->discard_text;
    if (ctx->bz.opt) ctx->bz.begin();
    *out_len = bz ? bgzf_text_room(need) : need;  // (a size query: out_capacity 0)
    if (!ctx->discard_text) {
        if (*out_len > out_capacity) {
            w.keep();  // (the window waits for the call the query sizes)
            return set_err(ctx, NTC_ERR_CAPACITY, bz ? "out_capacity smaller than the bound of the text's BGZF members"
                                                     : "out_capacity smaller than the FASTA text");
        }
        if (need && !out) return set_err(ctx, NTC_ERR_INVALID_ARG, "null argument");
    }
    ctx->pair.valid = ctx->pair.mode && !ctx->discard_text;
    ctx->pair.first = 0;
    if (ctx->unp_recs == 0) {
        if (bz) *out_len = 0;
        if (const int wrc = w.check(ctx->unp_reads)) return wrc;
        return ctx->unp_reads ? set_err(ctx, NTC_ERR_FORMAT, "reads without records") : NTC_OK;
    }
    return decode_fasta_dev(ctx, ctx->unp_d_recs, ctx->unp_recs, ctx->unp_reads, ctx->unp_bases, first_id, out, need, w,
                            out_len);
}

int ntc_decode_set_window(ntc_ctx *ctx, uint64_t first, uint64_t count) {
    if (!ctx) return NTC_ERR_INVALID_ARG;
    ctx->win.has_pending = false;
    // (the batch's reads are only known to the call that takes it: TextWindow::check)
    if (count == 0 || first + count < first) return set_err(ctx, NTC_ERR_INVALID_ARG, "an empty window");
    ctx->win.first = first;
    ctx->win.count = count;
    ctx->win.has_pending = true;
    return NTC_OK;
}

int ntc_decode_pair_split(ntc_ctx *ctx, uint64_t *first_bytes) {
    if (!ctx || !first_bytes) return set_err(ctx, NTC_ERR_INVALID_ARG, "null argument");
    *first_bytes = 0;
    if (!ctx->pair.valid) return set_err(ctx, NTC_ERR_INVALID_ARG, "the last text decode of this context was not a paired one");
    *first_bytes = ctx->pair.first;
    return NTC_OK;
}

int ntc_encode_exceptions(ntc_ctx *ctx, ntc_nx_run *out, uint64_t capacity, uint64_t *n_runs) {
    if (!ctx || !n_runs || (capacity && !out)) return set_err(ctx, NTC_ERR_INVALID_ARG, "null argument");
    *n_runs = ctx->nx.list.size();
    if (ctx->nx.list.size() > capacity) return set_err(ctx, NTC_ERR_CAPACITY, "capacity smaller than the exception runs");
    if (!ctx->nx.list.empty()) std::memcpy(out, ctx->nx.list.data(), ctx->nx.list.size() * sizeof(ntc_nx_run));
    return NTC_OK;
}

int ntc_decode_set_exceptions(ntc_ctx *ctx, const ntc_nx_run *runs, uint64_t n_runs, uint32_t sub) {
    if (!ctx || (n_runs && !runs)) return set_err(ctx, NTC_ERR_INVALID_ARG, "null argument");
    std::vector<ntc_nx_run> &p = ctx->nx.pending.metas;
    p.assign(runs, runs + n_runs);
    // each decode pass finds its runs by read: keep them in (read, pos) order (the canonical
    // lists already are)
    const auto less = [](const ntc_nx_run &a, const ntc_nx_run &b) { return a.read != b.read ? a.read < b.read : a.pos < b.pos; };
    if (!std::is_sorted(p.begin(), p.end(), less)) std::stable_sort(p.begin(), p.end(), less);
    ctx->nx.pending_sub = sub;
    ctx->nx.pending.has = n_runs != 0;
    return NTC_OK;
}

int ntc_encode_qualities(ntc_ctx *ctx, ntc_qual_meta *metas, uint64_t meta_cap, uint8_t *payload, uint64_t payload_cap,
                         uint64_t *n_blocks, uint64_t *payload_bytes) {
    if (!ctx || !n_blocks || !payload_bytes || (meta_cap && !metas) || (payload_cap && !payload))
        return set_err(ctx, NTC_ERR_INVALID_ARG, "null argument");
    *n_blocks = ctx->qual.blocks;
    *payload_bytes = ctx->qual.words * 8;
    if (ctx->qual.blocks > meta_cap || ctx->qual.words * 8 > payload_cap)
        return set_err(ctx, NTC_ERR_CAPACITY, "capacity smaller than the quality sections");
    if (ctx->qual.blocks == 0) return NTC_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint64_t nb = ctx->qual.blocks;
    std::vector<QBlock> blk(nb);
    HIP_TRY(ctx, hipMemcpy(blk.data(), (const uint8_t *)ctx->ws[WS_Q_BLOCKS].p + 64 + nb * 16, nb * sizeof(QBlock),
                           hipMemcpyDeviceToHost));
    if (ctx->qual.words)
        HIP_TRY(ctx, hipMemcpy(payload, ctx->ws[WS_Q_PAYLOAD].p, ctx->qual.words * 8, hipMemcpyDeviceToHost));
    for (uint64_t b = 0; b < nb; b++) {
        ntc_qual_meta &m = metas[b];
        std::memset(&m, 0, sizeof(m));
        m.n_reads = std::min<uint64_t>(ctx->qual.block_reads, ctx->qual.reads - b * ctx->qual.block_reads);
        m.n_quals = blk[b].n_quals;
        m.payload_off = blk[b].word_off * 8;
        m.payload_bytes = ctx->qual.coder_last == 1 ? blk[b].body_bytes : blk[b].n_words * 8;
        m.reserved[0] = (uint8_t)ctx->qual.coder_last;
        m.width = (uint8_t)blk[b].w;
        m.n_syms = (uint8_t)blk[b].n_syms;
        std::memcpy(m.alphabet, blk[b].alphabet, blk[b].n_syms);
    }
    return NTC_OK;
}

int ntc_decode_set_qualities(ntc_ctx *ctx, const ntc_qual_meta *metas, uint64_t n_blocks, const uint8_t *payload,
                             uint64_t payload_bytes) {
    if (!ctx || (n_blocks && !metas) || (payload_bytes && !payload)) return set_err(ctx, NTC_ERR_INVALID_ARG, "null argument");
    ctx->qual.pending.clear();
    if (n_blocks == 0) return NTC_OK;
    const uint32_t coder = metas[0].reserved[0];  // 0 pack, 1 rans: one coder for all sections
    if (coder > 1) return set_err(ctx, NTC_ERR_FORMAT, "quality sections of an unknown coder");
    if (coder == 0 && (payload_bytes & 7)) return set_err(ctx, NTC_ERR_FORMAT, "quality payload is not whole 64-bit words");
    for (uint64_t b = 0; b < n_blocks; b++) {
        const ntc_qual_meta &m = metas[b];
        if (!q_meta_ok(m.n_quals, m.width, m.n_syms, m.alphabet))
            return set_err(ctx, NTC_ERR_FORMAT, "quality section " + std::to_string(b) + ": width, n_syms or alphabet");
        if (m.reserved[0] != coder) return set_err(ctx, NTC_ERR_FORMAT, "quality sections of more than one coder");
        if (coder == 1) {
            if (m.n_quals >> 40 || (m.payload_off & 7) || m.payload_off > payload_bytes ||
                m.payload_bytes > payload_bytes - m.payload_off ||
                !qr_body_ok(m.n_quals, m.n_syms, payload + m.payload_off, m.payload_bytes))
                return set_err(ctx, NTC_ERR_FORMAT, "quality section " + std::to_string(b) + ": table, span sizes or place");
            continue;
        }
        if (m.n_quals >> 40 || m.payload_bytes != q_words(m.n_quals, m.width) * 8 || (m.payload_off & 7) ||
            m.payload_off > payload_bytes || m.payload_bytes > payload_bytes - m.payload_off)
            return set_err(ctx, NTC_ERR_FORMAT, "quality section " + std::to_string(b) + ": payload size or place");
    }
    ctx->qual.pending.metas.assign(metas, metas + n_blocks);
    ctx->qual.pending.payload.assign((payload_bytes + 7) / 8, 0);
    if (payload_bytes) std::memcpy(ctx->qual.pending.payload.data(), payload, payload_bytes);
    ctx->qual.pending.has = true;
    return NTC_OK;
}

int ntc_encode_names(ntc_ctx *ctx, ntc_name_meta *metas, uint64_t meta_cap, uint8_t *payload, uint64_t payload_cap,
                     uint64_t *n_blocks, uint64_t *payload_bytes) {
    if (!ctx || !n_blocks || !payload_bytes || (meta_cap && !metas) || (payload_cap && !payload))
        return set_err(ctx, NTC_ERR_INVALID_ARG, "null argument");
    *n_blocks = ctx->names.blocks;
    *payload_bytes = ctx->names.bytes;
    if (ctx->names.blocks > meta_cap || ctx->names.bytes > payload_cap)
        return set_err(ctx, NTC_ERR_CAPACITY, "capacity smaller than the name sections");
    if (ctx->names.blocks == 0) return NTC_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    static_assert(sizeof(NBlock) == sizeof(ntc_name_meta), "the device table is the public meta");
    HIP_TRY(ctx, hipMemcpy(metas, (const uint8_t *)ctx->ws[WS_N_BLOCKS].p + 64, ctx->names.blocks * sizeof(NBlock),
                           hipMemcpyDeviceToHost));
    if (ctx->names.bytes) HIP_TRY(ctx, hipMemcpy(payload, ctx->ws[WS_N_PAYLOAD].p, ctx->names.bytes, hipMemcpyDeviceToHost));
    return NTC_OK;
}

int ntc_decode_set_names(ntc_ctx *ctx, const ntc_name_meta *metas, uint64_t n_blocks, const uint8_t *payload,
                         uint64_t payload_bytes) {
    if (!ctx || (n_blocks && !metas) || (payload_bytes && !payload)) return set_err(ctx, NTC_ERR_INVALID_ARG, "null argument");
    ctx->names.pending.clear();
    if (n_blocks == 0) return NTC_OK;
    if (payload_bytes & 7) return set_err(ctx, NTC_ERR_FORMAT, "name payload is not a multiple of 8 bytes");
    for (uint64_t b = 0; b < n_blocks; b++) {
        const ntc_name_meta &m = metas[b];
        if (m.mid_bytes >> 48 || !n_meta_ok(m.n_reads, m.name_bytes, m.mid_bytes, m.payload_bytes))
            return set_err(ctx, NTC_ERR_FORMAT, "name section " + std::to_string(b) + ": counts or payload size");
        if ((m.payload_off & 7) || m.payload_off > payload_bytes || m.payload_bytes > payload_bytes - m.payload_off)
            return set_err(ctx, NTC_ERR_FORMAT, "name section " + std::to_string(b) + ": payload place");
    }
    ctx->names.pending.metas.assign(metas, metas + n_blocks);
    ctx->names.pending.payload.resize(payload_bytes / 8);
    if (payload_bytes) std::memcpy(ctx->names.pending.payload.data(), payload, payload_bytes);
    ctx->names.pending.has = true;
    return NTC_OK;
}

int ntc_encode_digests(ntc_ctx *ctx, ntc_digest_meta *metas, uint64_t cap, uint64_t *n_blocks) {
    if (!ctx || !n_blocks || (cap && !metas)) return set_err(ctx, NTC_ERR_INVALID_ARG, "null argument");
    *n_blocks = ctx->dig.blocks;
    if (ctx->dig.blocks > cap) return set_err(ctx, NTC_ERR_CAPACITY, "capacity smaller than the digest table");
    if (ctx->dig.blocks == 0) return NTC_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpy(metas, ctx->ws[WS_DG_TABLE].p, ctx->dig.blocks * sizeof(ntc_digest_meta), hipMemcpyDeviceToHost));
    return NTC_OK;
}

int ntc_decode_set_digests(ntc_ctx *ctx, const ntc_digest_meta *metas, uint64_t n_blocks) {
    if (!ctx || (n_blocks && !metas)) return set_err(ctx, NTC_ERR_INVALID_ARG, "null argument");
    ctx->dig.pending.clear();
    for (uint64_t b = 0; b < n_blocks; b++) {
        const ntc_digest_meta &m = metas[b];
        const uint64_t d[4] = {m.d_seq, m.d_sym, m.d_qual, m.d_name};
        if (!dg_meta_ok(m.components, m.reserved, d) || !m.n_reads || m.n_reads >> 32)
            return set_err(ctx, NTC_ERR_INVALID_ARG, "digest section " + std::to_string(b) + ": components, reads or a digest "
                                                     "of an absent component");
    }
    ctx->dig.pending.metas.assign(metas, metas + n_blocks);
    ctx->dig.pending.has = n_blocks != 0;
    return NTC_OK;
}

int ntc_decode_digests(ntc_ctx *ctx, ntc_digest_meta *metas, uint64_t cap, uint64_t *n_blocks) {
    if (!ctx || !n_blocks || (cap && !metas)) return set_err(ctx, NTC_ERR_INVALID_ARG, "null argument");
    *n_blocks = ctx->dig.computed.size();
    if (ctx->dig.computed.size() > cap) return set_err(ctx, NTC_ERR_CAPACITY, "capacity smaller than the digest table");
    if (!ctx->dig.computed.empty())
        std::memcpy(metas, ctx->dig.computed.data(), ctx->dig.computed.size() * sizeof(ntc_digest_meta));
    return NTC_OK;
}

int ntc_last_timing(ntc_ctx *ctx, ntc_timing *out) {
    if (!ctx || !out) return NTC_ERR_INVALID_ARG;
    if (ctx->last == kNone) return set_err(ctx, NTC_ERR_INVALID_ARG, "no call yet");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipEventSynchronize(ctx->ev[2]));
    float a = 0, b = 0;
    std::memset(out, 0, sizeof(*out));
    if ((ctx->last == kEncode && ctx->last_variant == 4) || ctx->last == kDecode) {
        // main = the dominant kernel alone: k_ms4 (ev[3] -> ev[1]) or k_dec_rec (ev[1] -> ev[3])
        float tot = 0, ms = 0;
        HIP_TRY(ctx, hipEventElapsedTime(&tot, ctx->ev[0], ctx->ev[2]));
        if (ctx->last == kDecode) HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev[1], ctx->ev[3]));
        else HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev[3], ctx->ev[1]));
        out->main_ms = ms;
        out->aux_ms = (double)tot - (double)ms;
        out->total_ms = tot;
        out->units = ctx->last_units;
        return NTC_OK;
    }
    HIP_TRY(ctx, hipEventElapsedTime(&a, ctx->ev[0], ctx->ev[1]));
    HIP_TRY(ctx, hipEventElapsedTime(&b, ctx->ev[1], ctx->ev[2]));
    if (ctx->last == kEncode) {
        out->main_ms = a;
        out->aux_ms = b;
    } else {
        out->aux_ms = a;
        out->main_ms = b;
    }
    out->total_ms = (double)a + (double)b;
    out->units = ctx->last_units;
    return NTC_OK;
}

int ntc_device_alloc(ntc_ctx *ctx, uint64_t bytes, void **d_ptr) {
    if (!ctx || !d_ptr) return NTC_ERR_INVALID_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMalloc(d_ptr, bytes ? bytes : 64));
    return NTC_OK;
}
int ntc_device_free(ntc_ctx *ctx, void *d_ptr) {
    if (!ctx) return NTC_ERR_INVALID_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipFree(d_ptr));
    return NTC_OK;
}
int ntc_memcpy_h2d(ntc_ctx *ctx, void *d_dst, const void *h_src, uint64_t bytes) {
    if (!ctx) return NTC_ERR_INVALID_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return NTC_OK;
}
int ntc_memcpy_d2h(ntc_ctx *ctx, void *h_dst, const void *d_src, uint64_t bytes) {
    if (!ctx) return NTC_ERR_INVALID_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return NTC_OK;
}

int ntc_debug_matching_statistics(ntc_ctx *ctx, const uint8_t *bases, const uint64_t *read_offsets,
                                  uint64_t n_reads, uint32_t *d_out, uint32_t *start_out) {
    if (!ctx || !read_offsets || !d_out || !start_out) return set_err(ctx, NTC_ERR_INVALID_ARG, "null argument");
    const uint64_t total = read_offsets[n_reads] - read_offsets[0];
    std::vector<uint64_t> recs(total + 1), roffs(n_reads + 1);
    int64_t bad = -1;
    int rc = ntc_encode_batch(ctx, bases, read_offsets, n_reads, recs.data(), total + 1, roffs.data(), &bad);
    if (rc && rc != NTC_ERR_LENGTH) return rc;
    if (ctx->encode_variant == 4) {
        void *dd, *ds;
        if ((rc = ensure(ctx, WS_DEC_A, (total + 1) * 4, &dd))) return rc;
        if ((rc = ensure(ctx, WS_DEC_B, (total + 1) * 4, &ds))) return rc;
        launch_debug_gather4(ctx->last4, (uint32_t *)dd, (uint32_t *)ds, ctx->stream);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        HIP_TRY(ctx, hipMemcpy(d_out, dd, total * 4, hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(start_out, ds, total * 4, hipMemcpyDeviceToHost));
        return NTC_OK;
    }
    DebugArgs g{};
    g.D = (const uint8_t *)ctx->ws[WS_D].p;
    g.S = (const uint32_t *)ctx->ws[WS_S].p;
    g.tile_base = (const uint64_t *)ctx->ws[WS_TILEBASE].p;
    g.offs = (const uint64_t *)ctx->ws[WS_STAGE_OFFS].p;
    g.n_reads = n_reads;
    void *dd, *ds;
    if ((rc = ensure(ctx, WS_DEC_A, (total + 1) * 4, &dd))) return rc;
    if ((rc = ensure(ctx, WS_DEC_B, (total + 1) * 4, &ds))) return rc;
    g.d_out = (uint32_t *)dd;
    g.s_out = (uint32_t *)ds;
    launch_debug_gather(g, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(d_out, dd, total * 4, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(start_out, ds, total * 4, hipMemcpyDeviceToHost));
    return NTC_OK;
}

// ---- host-side index producer / files ---------------------------------------------------
int ntc_build_index(const uint8_t *seqs, const uint64_t *seq_offsets, uint64_t n_seqs, uint32_t k,
                    int add_revcomp, int n_threads, ntc_index_host **out) {
    if (!out || !seq_offsets || (n_seqs && !seqs)) return NTC_ERR_INVALID_ARG;
    if (k < 1 || k > 255) return NTC_ERR_UNSUPPORTED;
    *out = nullptr;
    try {
        auto *h = new ntc_index_host();
        build_index(seqs, seq_offsets, n_seqs, k, add_revcomp != 0, n_threads, h->ix);
        *out = h;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "ntc_build_index: %s\n", e.what());
        return NTC_ERR_FORMAT;
    }
    return NTC_OK;
}

int ntc_build_index_device(ntc_ctx *ctx, const uint8_t *seqs, const uint64_t *seq_offsets, uint64_t n_seqs,
                           uint32_t k, int add_revcomp, ntc_index_host **out) {
    return ntc_build_index_device_ex(ctx, seqs, seq_offsets, n_seqs, k, add_revcomp, nullptr, nullptr, out);
}

int ntc_build_index_device_ex(ntc_ctx *ctx, const uint8_t *seqs, const uint64_t *seq_offsets, uint64_t n_seqs,
                              uint32_t k, int add_revcomp, const ntc_build_opts *opts, ntc_build_stats *stats,
                              ntc_index_host **out) {
    if (!ctx || !out || !seq_offsets || (n_seqs && !seqs)) return set_err(ctx, NTC_ERR_INVALID_ARG, "null argument");
    if (k < 1 || k > 255) return set_err(ctx, NTC_ERR_UNSUPPORTED, "k must be in [1, 255]");
    *out = nullptr;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    for (uint64_t i = 0; i < n_seqs; i++)
        if (seq_offsets[i + 1] < seq_offsets[i]) return set_err(ctx, NTC_ERR_INVALID_ARG, "sequence offsets decrease");
    BuildOpts o;
    if (opts) {
        o.device_budget = opts->device_budget_bytes;
        o.host_budget = opts->host_budget_bytes;
        o.max_partition_keys = opts->max_partition_keys;
        if (opts->temp_dir && *opts->temp_dir) o.temp_dir = opts->temp_dir;
    }
    if (o.temp_dir.empty()) {
        const char *t = std::getenv("TMPDIR");
        o.temp_dir = t && *t ? t : "/tmp";
    }
    auto *h = new ntc_index_host();
    std::string err;
    BuildStats st;
    const bool ok = build_index_device(ctx->stream, seqs, seq_offsets, n_seqs, k, add_revcomp != 0, o, h->ix, st, err);
    if (stats) {
        stats->occurrences = st.occurrences;
        stats->kmers = st.kmers;
        stats->sources = st.sources;
        stats->nodes = st.nodes;
        stats->spilled_bytes = st.spilled_bytes;
        stats->device_budget_bytes = st.device_budget;
        stats->pass_keys = st.pass_keys;
        stats->peak_device_bytes = st.peak_device_bytes;
        stats->kmer_partitions = st.kmer_partitions;
        stats->node_partitions = st.node_partitions;
        stats->compactions = st.compactions;
        stats->seq_uploads = st.seq_uploads;
        stats->seconds = st.seconds;
        stats->seconds_kmers = st.seconds_kmers;
        stats->seconds_sources = st.seconds_sources;
        stats->seconds_nodes = st.seconds_nodes;
        stats->seconds_labels = st.seconds_labels;
        stats->seconds_plan = st.seconds_plan;
        stats->seconds_sort = st.seconds_sort;
    }
    if (!ok) {
        delete h;
        const int code = err.rfind("hip", 0) == 0 ? NTC_ERR_HIP
                         : err.find("allocation") != std::string::npos || err.find("budget") != std::string::npos
                             ? NTC_ERR_CAPACITY
                         : err.find("temp-dir") != std::string::npos || err.find("partition file") != std::string::npos
                             ? NTC_ERR_IO
                             : NTC_ERR_FORMAT;
        return set_err(ctx, code, "ntc_build_index_device: " + err);
    }
    *out = h;
    return NTC_OK;
}

int ntc_index_set_prefix_precalc(ntc_index_host *ix, uint32_t p) {
    if (!ix || p > 12 || p > ix->ix.k) return NTC_ERR_INVALID_ARG;
    ix->ix.prefix_len = p;
    ix->ix.prefix_ranges.clear();
    if (p) prefix_table(ix->ix, p, ix->ix.prefix_ranges);
    return NTC_OK;
}

int ntc_index_prefix_table(const ntc_index_host *ix, uint32_t *p, uint64_t *ranges) {
    if (!ix || !p) return NTC_ERR_INVALID_ARG;
    *p = ix->ix.prefix_len;
    if (ranges && !ix->ix.prefix_ranges.empty())
        std::memcpy(ranges, ix->ix.prefix_ranges.data(), ix->ix.prefix_ranges.size() * 8);
    return NTC_OK;
}

void ntc_index_free(ntc_index_host *ix) { delete ix; }

int ntc_index_view_of(const ntc_index_host *ix, ntc_index_view *v) {
    if (!ix || !v) return NTC_ERR_INVALID_ARG;
    v->n_nodes = ix->ix.n;
    v->k = ix->ix.k;
    v->reserved = 0;
    for (int c = 0; c < 4; c++) {
        v->rows[c] = ix->ix.rows[c].data();
        v->C[c] = ix->ix.C[c];
    }
    v->lcs = ix->ix.lcs.data();
    return NTC_OK;
}

int ntc_index_save(const ntc_index_host *ix, const char *prefix) {
    if (!ix || !prefix) return NTC_ERR_INVALID_ARG;
    std::string err;
    if (!save_index(ix->ix, prefix, err)) {
        std::fprintf(stderr, "ntc_index_save: %s\n", err.c_str());
        return NTC_ERR_IO;
    }
    return NTC_OK;
}

int ntc_index_save_as(const ntc_index_host *ix, const char *prefix, int layout) {
    if (!ix || !prefix || (layout != kIndexOwn && layout != kIndexSbwtRs)) return NTC_ERR_INVALID_ARG;
    std::string err;
    if (!save_index_as(ix->ix, prefix, layout, err)) {
        std::fprintf(stderr, "ntc_index_save_as: %s\n", err.c_str());
        return NTC_ERR_IO;
    }
    return NTC_OK;
}

int ntc_index_load(const char *prefix, ntc_index_host **out) {
    if (!prefix || !out) return NTC_ERR_INVALID_ARG;
    *out = nullptr;
    auto *h = new ntc_index_host();
    std::string err;
    if (!load_index(prefix, h->ix, err)) {
        std::fprintf(stderr, "ntc_index_load: %s\n", err.c_str());
        delete h;
        return NTC_ERR_IO;
    }
    *out = h;
    return NTC_OK;
}

}  // extern "C"

// the pipelines' way to the non-ACGT entry points (ntc_internal.h NxHooks), set at load
namespace {
struct NxHookFill {
    NxHookFill() {
        ntc::g_nx_hooks.set_policy = [](ntc_ctx *ctx, int policy) { return ntc_ctx_set_option(ctx, "non_acgt", policy); };
        ntc::g_nx_hooks.last_counts = [](ntc_ctx *ctx, uint32_t *sub, uint64_t *runs, uint64_t *bases) {
            if (!ctx) return (int)NTC_ERR_INVALID_ARG;
            if (sub) *sub = ctx->has_index ? nx_substitute(ctx->dix.absent) : 0;
            if (runs) *runs = ctx->nx.runs;
            if (bases) *bases = ctx->nx.bases;
            return (int)NTC_OK;
        };
        ntc::g_nx_hooks.encode_exceptions = ntc_encode_exceptions;
        ntc::g_nx_hooks.decode_set_exceptions = ntc_decode_set_exceptions;
        ntc::g_p_hooks.set_mode = [](ntc_ctx *ctx, int mode) { return ntc_ctx_set_option(ctx, "paired", mode); };
        ntc::g_p_hooks.encode_paired = ntc_encode_pack_fastq_paired;
        ntc::g_p_hooks.pair_split = ntc_decode_pair_split;
        ntc::g_w_hooks.decode_set_window = ntc_decode_set_window;
        ntc::g_q_hooks.set_mode = [](ntc_ctx *ctx, int mode) { return ntc_ctx_set_option(ctx, "qualities", mode); };
        ntc::g_q_hooks.encode_qualities = ntc_encode_qualities;
        ntc::g_q_hooks.get_coder = [](ntc_ctx *ctx) {
            int64_t v = 0;
            return ntc_ctx_get_option(ctx, "quality_coder", &v) == NTC_OK ? (int)v : -1;
        };
        ntc::g_q_hooks.decode_set_qualities = ntc_decode_set_qualities;
        ntc::g_n_hooks.set_mode = [](ntc_ctx *ctx, int mode) { return ntc_ctx_set_option(ctx, "names", mode); };
        ntc::g_n_hooks.encode_names = ntc_encode_names;
        ntc::g_n_hooks.decode_set_names = ntc_decode_set_names;
        ntc::g_d_hooks.set_mode = [](ntc_ctx *ctx, int on) { return ntc_ctx_set_option(ctx, "digests", on); };
        ntc::g_d_hooks.encode_digests = ntc_encode_digests;
        ntc::g_d_hooks.decode_set_digests = ntc_decode_set_digests;
        ntc::g_d_hooks.decode_digests = ntc_decode_digests;
        ntc::g_d_hooks.index_info = [](ntc_ctx *ctx, uint64_t *n_nodes, uint32_t *k) {
            return ntc_index_info(ctx, n_nodes, k, nullptr);
        };
        ntc::g_d_hooks.set_discard = [](ntc_ctx *ctx, int on) { return ntc_ctx_set_option(ctx, "discard_text", on); };
        ntc::g_z_hooks.set_mode = [](ntc_ctx *ctx, int on) { return ntc_ctx_set_option(ctx, "gpu_deflate", on); };
        ntc::g_z_hooks.encode_members = ntc_encode_members;
        ntc::g_b_hooks.set_mode = [](ntc_ctx *ctx, int on) { return ntc_ctx_set_option(ctx, "bgzf_text", on); };
        ntc::g_b_hooks.last_counts = [](ntc_ctx *ctx, ntc_bgzf_counts *c) {
            uint64_t n = 0;
            return ntc_bgzf_last(ctx, c, nullptr, 0, &n);
        };
        ntc::g_i_hooks.create = [](ntc_ctx *ctx, ntc::Inflater **out) {
            if (!ctx || !out) return (int)NTC_ERR_INVALID_ARG;
            *out = nullptr;
            if (hipSetDevice(ctx->device) != hipSuccess) return set_err(ctx, NTC_ERR_HIP, "hipSetDevice");
            ntc::Inflater *inf = new ntc::Inflater;
            inf->device = ctx->device;
            if (hipStreamCreateWithFlags(&inf->stream, hipStreamNonBlocking) != hipSuccess) {
                inf->stream = nullptr;
                delete inf;
                return set_err(ctx, NTC_ERR_HIP, "the inflater's stream");
            }
            *out = inf;
            return (int)NTC_OK;
        };
        ntc::g_i_hooks.run = [](ntc::Inflater *inf, const uint8_t *comp, uint64_t comp_bytes, const ntc_inflate_member *m,
                                uint64_t n, uint8_t *dst, uint64_t dst_bytes, uint64_t *n_failed) {
            return inf->run(comp, comp_bytes, m, n, dst, dst_bytes, n_failed);
        };
        ntc::g_i_hooks.destroy = [](ntc::Inflater *inf) { delete inf; };
    }
} g_nx_hook_fill;
}  // namespace
