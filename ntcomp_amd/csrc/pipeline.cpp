// Native encode pipeline of the CLI: `ntcomp encode -i P reads.fq > encoded.dat`
// (src/main.rs:141-181), file in, encoded.dat out, with every stage overlapped:
//
//   reader   batches of blocks_per_batch x 65,536 reads (main.rs:152) into a ring of
//            pinned host buffers.  A plain FASTQ (mapped) goes as text: the reader's gang
//            copies it into the buffer while counting newlines and looking for blank lines
//            (fq_copy_scan), and cuts the batch after the last whole block's last line, so
//            the GPU parses it (ntc_encode_pack_fastq).  Anything else -- compressed input,
//            FASTA, a batch with a blank line from there on -- is parsed by the host pool
//            (ntc_fastx_next_batch_into); reads past the last whole block of a batch carry
//            into the next buffer.  Either way every block but the file's last holds
//            exactly 65,536 reads, and the last holds num_records % 65,536 (main.rs:174-177).
//   GPU      one driver thread per context, batches dealt round-robin:
//            ntc_encode_pack_fastq / ntc_encode_pack_batch = H2D, (parse,) encode kernels,
//            GPU block packer, D2H of the four coded streams per block (the u64 records
//            never leave HBM).
//   deflate  the host pool gzips each block's streams (ntc_deflate_block) -- the only
//            codec step left on the CPU.
//   writer   the calling thread writes the file header (lib.rs:52-67) and the blocks in
//            file order; a block the reference drops (no long or no short record,
//            write_block_to errs and main.rs:170 ignores it -- App. B.3) is skipped.
#include <emmintrin.h>
#include <hip/hip_runtime.h>
#include <sys/mman.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/ntcomp_codec.h"
#include "../../include/ntcomp_gpu.h"
#include "../../include/ntcomp_host.h"
#include "../../include/ntcomp_pipeline.h"
#include "ntc_internal.h"
#include "digest_core.h"

namespace ntc {
NxHooks g_nx_hooks = {nullptr, nullptr, nullptr, nullptr};  // capi.cpp fills it at load
QHooks g_q_hooks = {nullptr, nullptr, nullptr, nullptr};
NHooks g_n_hooks = {nullptr, nullptr, nullptr};
DHooks g_d_hooks = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
PHooks g_p_hooks = {nullptr, nullptr, nullptr};
}

namespace {

using Clock = std::chrono::steady_clock;
double secs(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double>(b - a).count(); }

// Pinned host memory: 2 MB pages, touched, then registered with HIP (hipHostRegister runs at
// ~25 GB/s, hipHostMalloc at ~4 GB/s on the box: scripts/ingest_bw.cpp, profiles/round4).
// Freed buffers stay registered in a process-wide pool (up to kPinnedPoolMax bytes) and are
// handed out again, so pipelines that grow and drop buffers per batch neither pay the
// registration again nor register a range the process just unregistered.
constexpr size_t kPinnedPoolMax = 8ull << 30;
struct PinnedPool {
    std::mutex mu;
    std::map<void *, size_t> size_of;       // every buffer handed out or pooled
    std::multimap<size_t, void *> idle;     // pooled: size -> buffer
    size_t idle_bytes = 0;
};
PinnedPool &pinned_pool() {
    static PinnedPool *p = new PinnedPool();  // never destroyed: buffers live until the process ends
    return *p;
}
// decode: the streams decoded on the host pool instead of the GPU (NTC_HOST_UNPACK=1)
bool host_unpack_on() {
    const char *h = std::getenv("NTC_HOST_UNPACK");
    return h && std::atoi(h) > 0;
}

void *pinned_alloc(size_t n) {
    const size_t sz = (std::max<size_t>(n, 1) + (2u << 20) - 1) & ~(size_t)((2u << 20) - 1);
    PinnedPool &P = pinned_pool();
    {
        std::lock_guard<std::mutex> g(P.mu);
        auto it = P.idle.lower_bound(sz);
        if (it != P.idle.end() && it->first <= 2 * sz + (64u << 20)) {  // not a far larger one
            void *q = it->second;
            P.idle_bytes -= it->first;
            P.idle.erase(it);
            return q;
        }
    }
    void *q = mmap(nullptr, sz, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (q == MAP_FAILED) return nullptr;
    madvise(q, sz, MADV_HUGEPAGE);
    std::memset(q, 0, sz);  // real pages before they are pinned
    if (hipHostRegister(q, sz, hipHostRegisterPortable) != hipSuccess) {
        (void)hipGetLastError();
        munmap(q, sz);
        return nullptr;
    }
    std::lock_guard<std::mutex> g(P.mu);
    P.size_of[q] = sz;
    return q;
}
void pinned_free(void *q) {
    if (!q) return;
    PinnedPool &P = pinned_pool();
    std::vector<std::pair<void *, size_t>> drop;
    {
        std::lock_guard<std::mutex> g(P.mu);
        auto it = P.size_of.find(q);
        if (it == P.size_of.end()) return;
        P.idle.emplace(it->second, q);
        P.idle_bytes += it->second;
        while (P.idle_bytes > kPinnedPoolMax && !P.idle.empty()) {  // the largest idle ones go
            auto big = std::prev(P.idle.end());
            drop.emplace_back(big->second, big->first);
            P.idle_bytes -= big->first;
            P.size_of.erase(big->second);
            P.idle.erase(big);
        }
    }
    for (auto &d : drop) {
        (void)hipHostUnregister(d.first);
        munmap(d.first, d.second);
    }
}

struct Batch {  // one pinned buffer of the ring
    uint8_t *bases = nullptr;
    uint64_t *offs = nullptr;
    uint64_t cap_bases = 0, cap_reads = 0;
    uint8_t *text = nullptr;  // plain FASTQ text for the GPU parse (text_len bytes, n_process records)
    uint64_t text_cap = 0, text_len = 0;
    bool is_text = false;
    bool is_pair = false;    // two mate texts: text_len bytes at text, text2_len bytes at text + text2_off
    uint64_t text2_off = 0, text2_len = 0;
    uint64_t n_reads = 0;    // reads in the buffer (carry + new)
    uint64_t n_process = 0;  // reads handed to the GPU (whole blocks, or all at the end)
    uint64_t first_read = 0; // file index of the buffer's first read
    uint64_t first_block = 0;
    bool busy = false;
};

// Copy n bytes of FASTQ text into dst (16-byte aligned) and scan them on the way: the
// newlines, and the first line inside the piece that starts with '\n' or '\r' (a blank
// line, which the host parser skips between records; the piece's first byte is the caller's).
struct FqScan {
    uint64_t nl = 0;
    size_t blank = SIZE_MAX;  // offset of the first blank line's first byte, or SIZE_MAX
};
template <bool kCopy>
FqScan fq_copy_scan(const uint8_t *src, uint8_t *dst, size_t n) {
    FqScan r;
    const __m128i NL = _mm_set1_epi8('\n'), CR = _mm_set1_epi8('\r');
    uint64_t carry = 0;  // the byte before this 64-byte block is '\n'
    size_t i = 0;
    for (; i + 64 <= n; i += 64) {
        uint64_t mnl = 0, mcr = 0;
        for (int k = 0; k < 4; k++) {
            const __m128i x = _mm_loadu_si128((const __m128i *)(src + i + 16 * k));
            if (kCopy) _mm_stream_si128((__m128i *)(dst + i + 16 * k), x);
            mnl |= (uint64_t)(uint32_t)_mm_movemask_epi8(_mm_cmpeq_epi8(x, NL)) << (16 * k);
            mcr |= (uint64_t)(uint32_t)_mm_movemask_epi8(_mm_cmpeq_epi8(x, CR)) << (16 * k);
        }
        const uint64_t bad = ((mnl << 1) | carry) & (mnl | mcr);
        if (bad && r.blank == SIZE_MAX) r.blank = i + (size_t)__builtin_ctzll(bad);
        carry = mnl >> 63;
        r.nl += (uint64_t)__builtin_popcountll(mnl);
    }
    if (kCopy) _mm_sfence();
    for (; i < n; i++) {
        const uint8_t c = src[i];
        if (kCopy) dst[i] = c;
        if (carry && (c == '\n' || c == '\r') && r.blank == SIZE_MAX) r.blank = i;
        carry = c == '\n';
        r.nl += c == '\n';
    }
    return r;
}

// byte position just past the target-th newline (1-based) of p[0, n), or n
size_t nth_newline_end(const uint8_t *p, size_t n, uint64_t target) {
    const __m128i NL = _mm_set1_epi8('\n');
    size_t i = 0;
    for (; i + 64 <= n; i += 64) {
        uint64_t m = 0;
        for (int k = 0; k < 4; k++)
            m |= (uint64_t)(uint32_t)_mm_movemask_epi8(_mm_cmpeq_epi8(_mm_loadu_si128((const __m128i *)(p + i + 16 * k)), NL))
                 << (16 * k);
        const uint64_t c = (uint64_t)__builtin_popcountll(m);
        if (c < target) {
            target -= c;
            continue;
        }
        for (; target > 1; target--) m &= m - 1;
        return i + (size_t)__builtin_ctzll(m) + 1;
    }
    for (; i < n; i++)
        if (p[i] == '\n' && --target == 0) return i + 1;
    return n;
}

struct BlockOut {  // a deflated block (its four streams' parts), or a dropped one
    uint8_t *part[4] = {nullptr, nullptr, nullptr, nullptr};
    uint64_t len[4] = {0, 0, 0, 0};
    int status = NTC_OK;
    int left = 0;  // parts not yet deflated
    uint64_t n_reads = 0;            // the block's reads
    std::vector<ntc_nx_run> nx;      // its exception runs (policy keep), read relative to the block
    bool has_q = false;              // quality mode keep / bin8: its section, deflated with the streams
    ntc_qual_meta qmeta{};
    uint8_t *qsec = nullptr;
    uint64_t qlen = 0;
    bool has_n = false;              // names mode keep / id: its section, likewise
    ntc_name_meta nmeta{};
    uint8_t *nsec = nullptr;
    uint64_t nlen = 0;
    bool has_d = false;              // digests on: its section of the "NTCD" file
    ntc_digest_meta dmeta{};
};

struct Shared {
    std::mutex mu;
    std::condition_variable cv;
    int error = NTC_OK;
    std::string msg;
    int64_t bad_read = -1;
    void fail(int code, const std::string &m, int64_t bad = -1) {
        std::lock_guard<std::mutex> g(mu);
        if (error == NTC_OK) {
            error = code;
            msg = m;
            bad_read = bad;
        }
        cv.notify_all();
    }
};

}  // namespace

extern "C" {

// policy / nx_fd / nx: ntc_encode_file_nx; ntc_encode_file passes policy -1 = the contexts as
// they are, no side file
// q_mode / q_fd / qs: ntc_encode_file_ex's quality side file (q_mode 0: none)
static int encode_file_impl(ntc_ctx *const *ctxs, int n_ctx, const char *in_path, int out_fd, int policy, int nx_fd,
                            const ntc_pipeline_opts *opts, ntc_pipeline_stats *stats, ntc_nx_stats *nx,
                            int q_mode = 0, int q_fd = -1, ntc_q_stats *qs = nullptr, int n_mode = 0, int n_fd = -1,
                            ntc_n_stats *ns = nullptr, int d_mode = 0, int d_fd = -1, ntc_d_stats *ds = nullptr,
                            int pair_mode = 0, const char *mate_path = nullptr, ntc_p_stats *ps = nullptr) {
    if (!ctxs || n_ctx <= 0 || !in_path || out_fd < 0) return NTC_ERR_INVALID_ARG;
    for (int i = 0; i < n_ctx; i++)
        if (!ctxs[i]) return NTC_ERR_INVALID_ARG;
    // pair_mode / mate_path / ps: ntc_encode_file_ex4's pairs (pair_mode 0: none)
    if (pair_mode < 0 || pair_mode > 2 || (!pair_mode && mate_path)) return NTC_ERR_INVALID_ARG;
    const ntc::PHooks &ph = ntc::g_p_hooks;
    if (pair_mode && (!ph.set_mode || !ph.encode_paired)) return NTC_ERR_UNSUPPORTED;
    ntc_p_stats PS{};
    PS.mode = (uint32_t)pair_mode;
    if (q_mode < 0 || q_mode > 2 || (q_mode ? q_fd < 0 : q_fd != -1)) return NTC_ERR_INVALID_ARG;
    const ntc::QHooks &qh = ntc::g_q_hooks;
    if (q_mode && (!qh.set_mode || !qh.encode_qualities)) return NTC_ERR_UNSUPPORTED;
    // the sections' coder is the contexts' "quality_coder" option, which must be the same in all
    int q_coder = 0;
    if (q_mode && qh.get_coder) {
        q_coder = qh.get_coder(ctxs[0]);
        for (int i = 0; i < n_ctx; i++)
            if (q_coder < 0 || qh.get_coder(ctxs[i]) != q_coder) return NTC_ERR_INVALID_ARG;
    }
    ntc_q_stats QS{};
    // n_mode / n_fd / ns: ntc_encode_file_ex2's name side file (n_mode 0: none)
    if (n_mode < 0 || n_mode > 2 || (n_mode ? n_fd < 0 : n_fd != -1)) return NTC_ERR_INVALID_ARG;
    const ntc::NHooks &nh = ntc::g_n_hooks;
    if (n_mode && (!nh.set_mode || !nh.encode_names)) return NTC_ERR_UNSUPPORTED;
    ntc_n_stats NS{};
    // d_mode / d_fd / ds: ntc_encode_file_ex3's digest side file (d_mode 0: none)
    if (d_mode < 0 || d_mode > 1 || (d_mode ? d_fd < 0 : d_fd != -1)) return NTC_ERR_INVALID_ARG;
    const ntc::DHooks &dh = ntc::g_d_hooks;
    if (d_mode && (!dh.set_mode || !dh.encode_digests || !dh.index_info)) return NTC_ERR_UNSUPPORTED;
    ntc_d_stats DS{};
    const bool keep = policy == NTC_NX_KEEP;
    ntc_nx_stats NX{};
    uint32_t nx_sub = 0;
    if (policy >= 0) {
        if (policy > NTC_NX_KEEP || (keep ? nx_fd < 0 : nx_fd != -1)) return NTC_ERR_INVALID_ARG;
        const ntc::NxHooks &hk = ntc::g_nx_hooks;
        if (policy != NTC_NX_ERROR && (!hk.set_policy || !hk.last_counts || !hk.encode_exceptions))
            return NTC_ERR_UNSUPPORTED;
        if (hk.set_policy)
            for (int i = 0; i < n_ctx; i++)
                if (int r = hk.set_policy(ctxs[i], policy)) return r;
        if (policy != NTC_NX_ERROR) {
            hk.last_counts(ctxs[0], &nx_sub, nullptr, nullptr);
            if (!nx_sub) {
                for (int i = 0; i < n_ctx; i++) hk.set_policy(ctxs[i], 0);
                return NTC_ERR_NO_INDEX;
            }
        }
    }
    struct PolicyReset {  // the contexts leave the call under policy error
        ntc_ctx *const *ctxs;
        int n;
        ~PolicyReset() {
            if (n > 0 && ntc::g_nx_hooks.set_policy)
                for (int i = 0; i < n; i++) ntc::g_nx_hooks.set_policy(ctxs[i], 0);
        }
    } policy_reset{ctxs, policy > 0 ? n_ctx : 0};
    if (q_mode)
        for (int i = 0; i < n_ctx; i++)
            if (int r = qh.set_mode(ctxs[i], q_mode)) {
                for (int j = 0; j < i; j++) qh.set_mode(ctxs[j], 0);
                return r;
            }
    struct ModeReset {  // ... and with qualities dropped
        ntc_ctx *const *ctxs;
        int n;
        ~ModeReset() {
            for (int i = 0; i < n; i++) ntc::g_q_hooks.set_mode(ctxs[i], 0);
        }
    } mode_reset{ctxs, q_mode ? n_ctx : 0};
    if (n_mode)
        for (int i = 0; i < n_ctx; i++)
            if (int r = nh.set_mode(ctxs[i], n_mode)) {
                for (int j = 0; j < i; j++) nh.set_mode(ctxs[j], 0);
                return r;
            }
    struct NamesReset {  // ... and with names dropped
        ntc_ctx *const *ctxs;
        int n;
        ~NamesReset() {
            for (int i = 0; i < n; i++) ntc::g_n_hooks.set_mode(ctxs[i], 0);
        }
    } names_reset{ctxs, n_mode ? n_ctx : 0};
    uint32_t d_k = 0;
    uint64_t d_nodes = 0;
    if (d_mode) {
        if (int r = dh.index_info(ctxs[0], &d_nodes, &d_k)) return r;
        for (int i = 0; i < n_ctx; i++)
            if (int r = dh.set_mode(ctxs[i], 1)) {
                for (int j = 0; j < i; j++) dh.set_mode(ctxs[j], 0);
                return r;
            }
    }
    struct DigestsReset {  // ... and with digests off
        ntc_ctx *const *ctxs;
        int n;
        ~DigestsReset() {
            for (int i = 0; i < n; i++) ntc::g_d_hooks.set_mode(ctxs[i], 0);
        }
    } digests_reset{ctxs, d_mode ? n_ctx : 0};
    if (pair_mode)
        for (int i = 0; i < n_ctx; i++)
            if (int r = ph.set_mode(ctxs[i], pair_mode)) {
                for (int j = 0; j < i; j++) ph.set_mode(ctxs[j], 0);
                return r;
            }
    struct PairsReset {  // ... and with pairs off
        ntc_ctx *const *ctxs;
        int n;
        ~PairsReset() {
            for (int i = 0; i < n; i++) ntc::g_p_hooks.set_mode(ctxs[i], 0);
        }
    } pairs_reset{ctxs, pair_mode ? n_ctx : 0};
    // the components the file can hold: what the modes of this call yield
    const uint32_t d_components = ntc::kDgSeq | (keep ? ntc::kDgSym : 0) | (q_mode ? ntc::kDgQual : 0) |
                                  (n_mode ? ntc::kDgName : 0);
    ntc_pipeline_opts o{};
    if (opts) o = *opts;
    const int T = o.threads > 0 ? o.threads : ntc_host_threads();
    const uint32_t BR = 65536;  // main.rs:152
    // 4 blocks per GPU call and 64 Mi-base buffers: the first batch is on the GPU after
    // ~30 ms and the pinned ring stays small (10 M x 150 bp: pipeline 0.59 -> 0.32 s against
    // 16 blocks and 256 Mi bases, scripts/pipe_bench.py on one MI355X box)
    const uint64_t per_batch = (uint64_t)(o.blocks_per_batch > 0 ? o.blocks_per_batch : 4) * BR;
    const uint64_t cap_bases = o.batch_bases > 0 ? o.batch_bases : (64ull << 20);
    const int engine = o.deflate_engine;
    ntc_pipeline_stats S{};
    const auto t0 = Clock::now();
    // NTC_PIPE_TRACE=n: the first n batches' (and blocks') events on stderr, ms from the start
    const char *etr = std::getenv("NTC_PIPE_TRACE");
    const uint64_t etrace_n = etr ? (uint64_t)std::atoll(etr) : 0;
    auto etrace = [&](const char *what, uint64_t b) {
        if (b < etrace_n) std::fprintf(stderr, "[pipe] %8.3f ms %s %llu\n", 1e3 * secs(t0, Clock::now()), what,
                                       (unsigned long long)b);
    };

    ntc_fastx *fx = nullptr;
    int rc = ntc_fastx_open(in_path, &fx);
    if (rc) return rc;
    ntc_fastx_set_threads(fx, T);
    // a mapped plain FASTQ goes to the GPU as text
    uint64_t text_n = 0;
    const uint8_t *text = o.host_parse ? nullptr : ntc::fastx_mapped(fx, &text_n);
    // the mate-2 input goes through the same ingest; the two decoders share the thread budget
    ntc_fastx *fx2 = nullptr;
    if (mate_path) {
        if ((rc = ntc_fastx_open(mate_path, &fx2))) {
            ntc_fastx_close(fx);
            return rc;
        }
        ntc_fastx_set_threads(fx, std::max(1, T / 2));
        ntc_fastx_set_threads(fx2, std::max(1, T / 2));
    }

    // pinned ring: the GPU threads hold at most n_ctx buffers, the reader fills one more.
    // A slot's base buffer (the large part, ~320 MB) is pinned by the reader when it first
    // fills the slot, so only the first one delays the first batch (pinning runs at a few
    // GB/s); the offsets are pinned here.
    const int NB = n_ctx + 2;
    std::vector<Batch> ring((size_t)NB);
    for (auto &b : ring) {
        b.cap_bases = cap_bases + BR * 1024ull;  // a carry of < 65,536 reads sits in front
        b.cap_reads = per_batch + BR + 1;
        if (!(b.offs = (uint64_t *)pinned_alloc(b.cap_reads * 8))) {
            for (auto &x : ring) pinned_free(x.offs);
            ntc_fastx_close(fx);
            if (fx2) ntc_fastx_close(fx2);
            return NTC_ERR_HIP;
        }
    }
    std::atomic<double> t_pin{0};
    S.alloc_s = secs(t0, Clock::now());
    Shared sh;
    std::vector<std::deque<int>> gpu_q((size_t)n_ctx);  // per context: ring indices in batch order
    bool reader_done = false;
    uint64_t total_blocks = 0;    // known once the reader is done
    std::atomic<double> t_parse{0}, t_gpu{0}, t_deflate{0}, t_write{0};
    // deflate tasks (one per stream of a block: ntc_deflate_stream) and blocks in progress
    struct Task {
        std::shared_ptr<uint8_t> payload;  // the GPU call's host payload (ntc_buffer_free)
        ntc_block_meta meta;
        uint64_t block;
        int stream;                        // 0..3, 4 = the block's quality section, 5 = its name section
        std::shared_ptr<uint8_t> qpayload = nullptr;  // the call's packed quality words (4), name sections (5)
    };
    std::deque<Task> tasks;
    std::map<uint64_t, BlockOut> done;
    uint64_t pending_tasks = 0;
    uint64_t writer_at = 0;  // the block the writer waits for
    const uint64_t max_pending = (uint64_t)T * 8 + 64;  // bound on blocks queued or finished but unwritten

    auto add_time = [](std::atomic<double> &a, double d) {
        double cur = a.load();
        while (!a.compare_exchange_weak(cur, cur + d)) {
        }
    };

    // ---- reader ---------------------------------------------------------------------------
    // A buffer that cannot hold a whole 65,536-read block (long reads) grows until it does.
    auto grow = [&](Batch &b, uint64_t need_bases, uint64_t keep_bases, uint64_t keep_reads) -> bool {
        if (need_bases <= b.cap_bases) return true;
        const uint64_t cap = std::max(need_bases, b.cap_bases * 2);
        uint8_t *nbuf = (uint8_t *)pinned_alloc(cap);
        if (!nbuf) return false;
        if (keep_bases) std::memcpy(nbuf, b.bases, keep_bases);
        pinned_free(b.bases);
        b.bases = nbuf;
        b.cap_bases = cap;
        (void)keep_reads;
        return true;
    };
    // GPU-parse reader state.  Mapped: the next batch's text starts at text_pos (a record
    // start).  Streamed (a decoder's output): the text after the last cut, carry_n bytes at
    // carry_p in the previous batch's buffer, goes first into the next one.
    const bool streamed = !text && !o.host_parse && ntc::fastx_streamed_fastq(fx);
    // qualities exist only where the GPU parses the text (DESIGN.md "Quality scores")
    if (q_mode && o.host_parse)
        sh.fail(NTC_ERR_UNSUPPORTED, "qualities: host_parse = 1 parses on the host, which drops the quality lines");
    else if (q_mode && !text && !streamed)
        sh.fail(NTC_ERR_UNSUPPORTED, "qualities: the input is not FASTQ (FASTA has no quality lines)");
    // ... and so do names (DESIGN.md "Read names")
    if (n_mode && o.host_parse)
        sh.fail(NTC_ERR_UNSUPPORTED, "names: host_parse = 1 parses on the host, which drops the header lines");
    else if (n_mode && !text && !streamed)
        sh.fail(NTC_ERR_UNSUPPORTED, "names: the input is not FASTQ (names are kept from FASTQ text only)");
    // ... and so do pairs (DESIGN.md "Paired-end reads"): both inputs must reach the GPU as text
    struct TextSrc {  // one FASTQ input of the pair reader
        ntc_fastx *fx = nullptr;
        const uint8_t *map = nullptr;  // mapped plain text; null: streamed from a decoder
        uint64_t map_n = 0, pos = 0;   // mapped: the next record's start
        std::vector<uint8_t> pend;     // streamed: decoded text not yet sent
        bool at_end = false;           // streamed: the decoder has ended
        uint64_t sent = 0;             // text bytes sent so far
    } msrc[2];
    if (pair_mode && o.host_parse) {
        sh.fail(NTC_ERR_UNSUPPORTED, "pairs: host_parse = 1 parses on the host, which drops the header lines");
    } else if (pair_mode && !text && !streamed) {
        sh.fail(NTC_ERR_UNSUPPORTED, "pairs: the input is not FASTQ (mates are checked and woven in FASTQ text only)");
    } else if (mate_path) {
        msrc[0].fx = fx;
        msrc[0].map = text;
        msrc[0].map_n = text_n;
        msrc[1].fx = fx2;
        msrc[1].map = ntc::fastx_mapped(fx2, &msrc[1].map_n);
        if (!msrc[1].map && !ntc::fastx_streamed_fastq(fx2))
            sh.fail(NTC_ERR_UNSUPPORTED, "pairs: the mate input is not FASTQ (mates are checked and woven in FASTQ text only)");
    }
    uint64_t text_pos = 0;
    const uint8_t *carry_p = nullptr;
    uint64_t carry_n = 0;
    bool stream_eof = false;
    double rec_bytes = 320;  // text bytes per record so far (a guess for 150 bp reads until known)
    std::atomic<uint64_t> text_batches{0};
    // the reader's gang: 8 threads copy + scan at ~45 GB/s on the box, as fast as 16 for the
    // pipeline and at less CPU beside the deflate pool (scripts/rt_sweep.sh); NTC_READ_THREADS
    // is the A/B hook
    const char *rt_env = std::getenv("NTC_READ_THREADS");
    const int RT = std::max(1, rt_env ? std::atoi(rt_env) : std::min(T, 8));
    if (text) {  // bytes per record from the first MiB
        const size_t m = (size_t)std::min<uint64_t>(text_n, 1u << 20);
        uint64_t nl = 0;
        for (size_t i = 0; i < m; i++) nl += text[i] == '\n';
        rec_bytes = nl >= 4 ? 4.0 * (double)m / (double)nl : (double)m + 1;
    }
    // Fill b with the text of the next whole blocks (or the input's end): 1 = filled, 0 = no
    // input left, -1 = hand over to the host parser (a blank line before the cut, a line
    // count that is not a multiple of 4 at the end, a block too large for one call), -2 = the
    // decoder failed
    auto fill_text = [&](ntc::Gang &gang, Batch &b, bool &eof) -> int {
        const uint64_t kMaxText = (1ull << 32) - (64u << 20);  // ntc_encode_pack_fastq takes < 4 GiB
        uint64_t want_cap = (uint64_t)((double)per_batch * rec_bytes * 1.03) + (256u << 10);
        std::vector<FqScan> sc;
        for (;;) {
            if (!streamed) {
                if (text_pos >= text_n) return 0;
                if (text[text_pos] != '@') return -1;
            }
            // room for the carried text plus more (a batch read with a doubled buffer can leave a
            // carry larger than this batch's estimate)
            if (streamed) want_cap = std::max<uint64_t>(want_cap, carry_n + (4u << 20));
            want_cap = std::min(want_cap, kMaxText);
            if (streamed && carry_n >= want_cap) return -1;  // more than 4 GiB without one block
            if (b.text_cap < want_cap) {
                const auto ta = Clock::now();
                uint8_t *nt = (uint8_t *)pinned_alloc(want_cap);
                if (!nt) return -1;
                if (carry_n && carry_p == b.text) {  // growing the buffer that holds the carry
                    std::memcpy(nt, carry_p, carry_n);
                    carry_p = nt;
                }
                pinned_free(b.text);
                b.text = nt;
                b.text_cap = want_cap;
                t_pin = t_pin.load() + secs(ta, Clock::now());
            }
            uint64_t len;
            const uint8_t *src;
            if (!streamed) {
                len = std::min(text_n - text_pos, want_cap);
                src = text + text_pos;
            } else {
                if (carry_n && carry_p != b.text) std::memcpy(b.text, carry_p, carry_n);
                bool io_err = false;
                len = carry_n + ntc::fastx_stream_read(fx, b.text + carry_n, want_cap - carry_n, &io_err);
                if (io_err) return -2;
                stream_eof = len < want_cap;
                carry_p = b.text;  // all of it unused until the cut
                carry_n = len;
                if (len == 0) return 0;
                if (b.text[0] != '@') return -1;
                src = b.text;
            }
            constexpr uint64_t kPiece = 1u << 20;
            const uint64_t np = (len + kPiece - 1) / kPiece;
            sc.assign(np, FqScan{});
            std::atomic<uint64_t> next{0};
            gang.run([&](int) {
                for (uint64_t q; (q = next.fetch_add(1)) < np;) {
                    const uint64_t a = q * kPiece, e = std::min(len, a + kPiece);
                    sc[q] = streamed ? fq_copy_scan<false>(src + a, nullptr, e - a)
                                     : fq_copy_scan<true>(src + a, b.text + a, e - a);
                }
            });
            uint64_t nl = 0, blank = UINT64_MAX;  // the first blank line in the text read
            for (uint64_t q = 0; q < np; q++) {
                const uint64_t a = q * kPiece;
                if (blank == UINT64_MAX && a && src[a - 1] == '\n' && (src[a] == '\n' || src[a] == '\r')) blank = a;
                if (blank == UINT64_MAX && sc[q].blank != SIZE_MAX) blank = a + sc[q].blank;
                nl += sc[q].nl;
            }
            eof = streamed ? stream_eof : text_pos + len == text_n;
            // the text read ends the input with whole records and no blank line: all of it
            // goes; otherwise whole blocks of the complete records, cut after the last one's
            // last line
            const uint64_t lines = nl + (eof && src[len - 1] != '\n');
            const bool whole = eof && lines % 4 == 0 && blank == UINT64_MAX;
            const uint64_t recs = whole ? lines / 4 : nl / 4;
            uint64_t n = 0, cut = len;
            if (whole && recs <= per_batch) {
                n = recs;
            } else {
                n = std::min<uint64_t>(recs, per_batch) / BR * BR;
                if (n == 0) {  // not one whole block in the text read: read more, or give up
                    if (eof || len < want_cap || want_cap >= kMaxText) return -1;
                    want_cap *= 2;
                    continue;
                }
                // the batch ends after newline 4 n: find the piece holding it
                uint64_t before = 0, q = 0;
                while (before + sc[q].nl < 4 * n) before += sc[q++].nl;
                const uint64_t a = q * kPiece;
                cut = a + nth_newline_end(src + a, std::min(len, a + kPiece) - a, 4 * n - before);
                eof = false;
            }
            if (blank < cut) return -1;  // the batch holds a blank line: the host parser takes it
            b.text_len = cut;
            b.n_reads = b.n_process = n;
            rec_bytes = (double)cut / (double)std::max<uint64_t>(n, 1);
            if (streamed) {
                carry_p = b.text + cut;
                carry_n = len - cut;
                eof = eof || (stream_eof && carry_n == 0);
            } else {
                text_pos += cut;
                eof = eof || text_pos == text_n;
            }
            return 1;
        }
    };
    // The same for two mate inputs (mate_path): the next n records of each, the same n from
    // both -- 2 n a multiple of 65,536, or the inputs' end -- into b's one pinned buffer at two
    // offsets, for the GPU to weave.  The host newline counts make the cuts exact.  1 = filled,
    // 0 = no input left, -1 = a text the GPU cannot take (as above), -2 = a decoder failed, -3 =
    // one input ended while the other still holds a record
    auto fill_pair = [&](ntc::Gang &gang, Batch &b, bool &eof) -> int {
        const uint64_t kMaxHalf = ((1ull << 32) - (64u << 20)) / 2;  // both texts in one call of < 4 GiB
        const uint64_t half = per_batch / 2;
        constexpr uint64_t kPiece = 1u << 20;
        struct Win {
            const uint8_t *p = nullptr;
            uint64_t len = 0, recs = 0, blank = UINT64_MAX, cut = 0;
            bool end = false;
            std::vector<FqScan> sc;
        } w[2];
        for (int s = 0; s < 2; s++) {
            TextSrc &src = msrc[s];
            uint64_t want = std::min(kMaxHalf, (uint64_t)((double)half * rec_bytes * 1.03) + (256u << 10));
            for (;;) {
                if (src.map) {
                    w[s].p = src.map + src.pos;
                    w[s].len = std::min(src.map_n - src.pos, want);
                    w[s].end = src.pos + w[s].len == src.map_n;
                } else {
                    while (src.pend.size() < want && !src.at_end) {
                        const uint64_t old = src.pend.size();
                        src.pend.resize(want);
                        bool io_err = false;
                        const uint64_t got = ntc::fastx_stream_read(src.fx, src.pend.data() + old, want - old, &io_err);
                        if (io_err) return -2;
                        src.pend.resize(old + got);
                        src.at_end = got < want - old;
                    }
                    w[s].p = src.pend.data();
                    w[s].len = std::min<uint64_t>(src.pend.size(), want);
                    w[s].end = src.at_end && w[s].len == src.pend.size();
                }
                Win &x = w[s];
                x.recs = 0;
                if (x.len == 0) break;
                if (x.p[0] != '@') return -1;
                const uint64_t np = (x.len + kPiece - 1) / kPiece;
                x.sc.assign(np, FqScan{});
                std::atomic<uint64_t> next{0};
                gang.run([&](int) {
                    for (uint64_t q; (q = next.fetch_add(1)) < np;) {
                        const uint64_t a = q * kPiece, e = std::min(x.len, a + kPiece);
                        x.sc[q] = fq_copy_scan<false>(x.p + a, nullptr, e - a);
                    }
                });
                uint64_t nl = 0;
                x.blank = UINT64_MAX;
                for (uint64_t q = 0; q < np; q++) {
                    const uint64_t a = q * kPiece;
                    if (x.blank == UINT64_MAX && a && x.p[a - 1] == '\n' && (x.p[a] == '\n' || x.p[a] == '\r')) x.blank = a;
                    if (x.blank == UINT64_MAX && x.sc[q].blank != SIZE_MAX) x.blank = a + x.sc[q].blank;
                    nl += x.sc[q].nl;
                }
                const uint64_t lines = nl + (x.end && x.p[x.len - 1] != '\n');
                if (x.end && lines % 4 != 0) return -1;  // records that are not four lines each
                x.recs = x.end ? lines / 4 : nl / 4;
                if (x.recs >= half || x.end) break;
                if (want >= kMaxHalf) return -1;  // half of 4 GiB without half a batch
                want = std::min(want * 2, kMaxHalf);
            }
        }
        if (w[0].len == 0 && w[1].len == 0) return 0;
        const bool last = w[0].end && w[1].end && w[0].recs == w[1].recs && w[0].recs <= half;
        // an input that is not at its end holds at least half a batch here
        for (int s = 0; s < 2; s++)
            if (!last && w[s].end && w[s].recs < half && w[1 - s].recs > w[s].recs) return -3;
        const uint64_t n = last ? w[0].recs : half;
        for (int s = 0; s < 2; s++) {
            Win &x = w[s];
            x.cut = x.len;
            if (!last && !(x.end && x.recs == n)) {  // the batch ends after newline 4 n: find the piece holding it
                uint64_t before = 0, q = 0;
                while (before + x.sc[q].nl < 4 * n) before += x.sc[q++].nl;
                const uint64_t a = q * kPiece;
                x.cut = a + nth_newline_end(x.p + a, std::min(x.len, a + kPiece) - a, 4 * n - before);
            }
            if (x.blank < x.cut) return -1;  // a blank line: only the host parser takes it
        }
        const uint64_t at2 = (w[0].cut + 63) & ~63ull, need = at2 + w[1].cut + 64;
        if (b.text_cap < need) {
            const auto ta = Clock::now();
            uint8_t *nt = (uint8_t *)pinned_alloc(need + need / 8);
            if (!nt) return -1;
            pinned_free(b.text);
            b.text = nt;
            b.text_cap = need + need / 8;
            t_pin = t_pin.load() + secs(ta, Clock::now());
        }
        {  // both texts into the pinned buffer, piece by piece
            const uint64_t np0 = (w[0].cut + kPiece - 1) / kPiece, np1 = (w[1].cut + kPiece - 1) / kPiece;
            std::atomic<uint64_t> next{0};
            gang.run([&](int) {
                for (uint64_t q; (q = next.fetch_add(1)) < np0 + np1;) {
                    const int s = q < np0 ? 0 : 1;
                    const uint64_t a = (s ? q - np0 : q) * kPiece, e = std::min(w[s].cut, a + kPiece);
                    std::memcpy(b.text + (s ? at2 : 0) + a, w[s].p + a, e - a);
                }
            });
        }
        b.text_len = w[0].cut;
        b.text2_off = at2;
        b.text2_len = w[1].cut;
        b.n_reads = b.n_process = 2 * n;
        rec_bytes = (double)std::max(w[0].cut, w[1].cut) / (double)std::max<uint64_t>(n, 1);
        for (int s = 0; s < 2; s++) {
            TextSrc &src = msrc[s];
            src.sent += w[s].cut;
            if (src.map) src.pos += w[s].cut;
            else src.pend.erase(src.pend.begin(), src.pend.begin() + (ptrdiff_t)w[s].cut);
        }
        eof = last;
        return 1;
    };
    std::thread reader([&] {
        uint64_t next_read = 0, next_block = 0, batch_no = 0;
        int prev = -1;
        uint64_t carry = 0;  // reads at the tail of ring[prev] past its processed blocks
        bool as_text = text != nullptr || streamed || mate_path;  // (a mate input that is no text failed above)
        std::unique_ptr<ntc::Gang> gang(as_text ? new ntc::Gang(RT) : nullptr);
        for (;;) {
            int bi;
            {
                std::unique_lock<std::mutex> g(sh.mu);
                bi = (int)(batch_no % (uint64_t)NB);
                sh.cv.wait(g, [&] { return sh.error != NTC_OK || !ring[(size_t)bi].busy; });
                if (sh.error != NTC_OK) break;
            }
            Batch &b = ring[(size_t)bi];
            b.is_text = b.is_pair = false;
            if (as_text) {
                const auto tp = Clock::now();
                bool eof = false;
                const int r = mate_path ? fill_pair(*gang, b, eof) : fill_text(*gang, b, eof);
                add_time(t_parse, secs(tp, Clock::now()));
                if (r > 0) {
                    if (batch_no == 0) S.first_batch_s = secs(t0, Clock::now());
                    b.is_text = true;
                    b.is_pair = mate_path != nullptr;
                    b.first_read = next_read;
                    b.first_block = next_block;
                    next_read += b.n_process;
                    next_block += (b.n_process + BR - 1) / BR;
                    text_batches++;
                    etrace("read batch", batch_no);
                    {
                        std::lock_guard<std::mutex> g(sh.mu);
                        b.busy = true;
                        gpu_q[(size_t)(batch_no % (uint64_t)n_ctx)].push_back(bi);
                        batch_no++;
                        sh.cv.notify_all();
                    }
                    if (eof) break;
                    continue;
                }
                if (r == 0) break;
                if (r == -2) {
                    sh.fail(NTC_ERR_IO, "FASTX input: malformed or unreadable");
                    break;
                }
                if (r == -3) {
                    sh.fail(NTC_ERR_FORMAT, "mate files hold different numbers of records", (int64_t)next_read);
                    break;
                }
                if (pair_mode) {
                    sh.fail(NTC_ERR_UNSUPPORTED, "pairs: a blank line, or records that are not four lines each: "
                                                 "this batch needs the host parser, which drops the header lines",
                            (int64_t)next_read);
                    break;
                }
                if (q_mode) {
                    sh.fail(NTC_ERR_UNSUPPORTED, "qualities: a blank line, or records that are not four lines each: "
                                                 "this batch needs the host parser, which drops the quality lines",
                            (int64_t)next_read);
                    break;
                }
                if (n_mode) {
                    sh.fail(NTC_ERR_UNSUPPORTED, "names: a blank line, or records that are not four lines each: "
                                                 "this batch needs the host parser, which drops the header lines",
                            (int64_t)next_read);
                    break;
                }
                as_text = false;  // the host parser goes on from the first record not sent
                if (streamed) {
                    ntc::fastx_stream_unread(fx, carry_p, carry_n);
                    carry_n = 0;
                } else {
                    ntc::fastx_seek_mapped(fx, text_pos);
                }
            }
            if (!b.bases) {
                const auto ta = Clock::now();
                if (!(b.bases = (uint8_t *)pinned_alloc(b.cap_bases))) {
                    sh.fail(NTC_ERR_HIP, "pinned host allocation failed");
                    break;
                }
                t_pin = t_pin.load() + secs(ta, Clock::now());  // the reader alone writes it
            }
            uint64_t used = 0;  // bases in b
            b.offs[0] = 0;
            if (carry) {  // the previous buffer's unprocessed reads go first
                const Batch &p = ring[(size_t)prev];
                const uint64_t a0 = p.offs[p.n_process], a1 = p.offs[p.n_reads];
                if (!grow(b, (a1 - a0) * 2 + (64u << 20), 0, 0)) {
                    sh.fail(NTC_ERR_CAPACITY, "pinned host allocation failed");
                    break;
                }
                std::memcpy(b.bases, p.bases + a0, a1 - a0);
                for (uint64_t r = 0; r <= carry; r++) b.offs[r] = p.offs[p.n_process + r] - a0;
                used = a1 - a0;
            }
            b.n_reads = carry;
            bool eof = false, bad = false;
            const auto tp = Clock::now();
            for (;;) {  // fill: at least one whole block (or the end of the input)
                const uint64_t room = b.cap_bases - used;
                const uint64_t want = per_batch - b.n_reads, max_b = room / 2;
                uint64_t got = 0;
                const int r = ntc_fastx_next_batch_into(fx, want, max_b, b.bases + used, room, b.offs + b.n_reads, &got);
                if (r) {
                    sh.fail(r, r == NTC_ERR_CAPACITY ? "a read longer than half the batch buffer (raise batch_bases)"
                                                     : "FASTX input: malformed or unreadable");
                    bad = true;
                    break;
                }
                if (used)
                    for (uint64_t i = 0; i <= got; i++) b.offs[b.n_reads + i] += used;
                b.n_reads += got;
                const uint64_t nb = b.offs[b.n_reads] - used;
                used = b.offs[b.n_reads];
                if (got == 0 || (got < want && nb < max_b)) {
                    eof = true;
                    break;
                }
                if (b.n_reads >= BR || b.n_reads == per_batch) break;
                // fewer than 65,536 reads filled half the buffer: grow it and read on
                if (!grow(b, b.cap_bases * 2, used, b.n_reads)) {
                    sh.fail(NTC_ERR_CAPACITY, "pinned host allocation failed");
                    bad = true;
                    break;
                }
            }
            add_time(t_parse, secs(tp, Clock::now()));
            if (bad) break;
            if (batch_no == 0) S.first_batch_s = secs(t0, Clock::now());
            b.n_process = eof ? b.n_reads : (b.n_reads / BR) * BR;
            b.first_read = next_read;
            b.first_block = next_block;
            const uint64_t nblk = (b.n_process + BR - 1) / BR;
            carry = b.n_reads - b.n_process;
            prev = bi;
            next_read += b.n_process;
            next_block += nblk;
            if (b.n_process) {
                std::lock_guard<std::mutex> g(sh.mu);
                b.busy = true;
                gpu_q[(size_t)(batch_no % (uint64_t)n_ctx)].push_back(bi);
                batch_no++;
                sh.cv.notify_all();
            }
            if (eof && carry == 0) break;
        }
        std::lock_guard<std::mutex> g(sh.mu);
        S.reader_done_s = secs(t0, Clock::now());
        reader_done = true;
        total_blocks = next_block;
        S.reads = next_read;
        sh.cv.notify_all();
    });

    // ---- GPU drivers --------------------------------------------------------------------------
    std::vector<std::thread> gpus;
    for (int c = 0; c < n_ctx; c++)
        gpus.emplace_back([&, c] {
            for (;;) {
                int bi;
                {
                    std::unique_lock<std::mutex> g(sh.mu);
                    sh.cv.wait(g, [&] { return sh.error != NTC_OK || !gpu_q[(size_t)c].empty() || reader_done; });
                    if (sh.error != NTC_OK) return;
                    if (gpu_q[(size_t)c].empty()) {
                        if (reader_done) return;
                        continue;
                    }
                    bi = gpu_q[(size_t)c].front();
                    gpu_q[(size_t)c].pop_front();
                    // backpressure: do not run far ahead of the deflate pool and writer (the
                    // batch holding the writer's next block always goes)
                    sh.cv.wait(g, [&] {
                        return sh.error != NTC_OK || pending_tasks < max_pending ||
                               ring[(size_t)bi].first_block <= writer_at;
                    });
                    if (sh.error != NTC_OK) return;
                }
                Batch &b = ring[(size_t)bi];
                const uint64_t nblk = (b.n_process + BR - 1) / BR;
                std::vector<ntc_block_meta> metas(nblk);
                uint8_t *payload = nullptr;
                uint64_t plen = 0;
                int64_t bad = -1;
                uint64_t nb = 0;
                const auto tg = Clock::now();
                if (pair_mode && (b.n_process & 1)) {  // (only the input's last batch can be odd)
                    sh.fail(NTC_ERR_FORMAT, "pairs: an odd number of reads in an interleaved input", (int64_t)(b.first_read + b.n_process - 1));
                    return;
                }
                const int r = b.is_pair ? ph.encode_paired(ctxs[c], b.text, b.text_len, b.text + b.text2_off, b.text2_len,
                                                           b.n_process / 2, BR, metas.data(), &payload, &plen, &nb, &bad)
                              : b.is_text ? ntc_encode_pack_fastq(ctxs[c], b.text, b.text_len, b.n_process, BR,
                                                                  metas.data(), &payload, &plen, &nb, &bad)
                                          : ntc_encode_pack_batch(ctxs[c], b.bases, b.offs, b.n_process, BR,
                                                                  metas.data(), &payload, &plen, &bad);
                add_time(t_gpu, secs(tg, Clock::now()));
                if (r) {
                    ntc_buffer_free(payload);
                    if (b.is_text && r == NTC_ERR_FORMAT && !q_mode && !n_mode && !pair_mode)  // as the host parser reports it
                        sh.fail(r, "FASTX input: malformed or unreadable");
                    else
                        sh.fail(r, std::string("encode: ") + ntc_last_error(ctxs[c]),
                                bad >= 0 ? (int64_t)b.first_read + bad : -1);
                    return;
                }
                std::shared_ptr<uint8_t> pl(payload, ntc_buffer_free);
                // the batch's exception runs (policy keep) and counts, before the context's next call
                std::vector<ntc_nx_run> runs;
                uint64_t nx_runs = 0, nx_bases = 0;
                if (policy > 0) {
                    const ntc::NxHooks &hk = ntc::g_nx_hooks;
                    hk.last_counts(ctxs[c], nullptr, &nx_runs, &nx_bases);
                    uint64_t nrun = 0;
                    int rx = NTC_OK;
                    if (keep && hk.encode_exceptions(ctxs[c], nullptr, 0, &nrun) == NTC_ERR_CAPACITY) {
                        runs.resize(nrun);
                        rx = hk.encode_exceptions(ctxs[c], runs.data(), nrun, &nrun);
                    }
                    if (rx) {
                        sh.fail(rx, std::string("encode: ") + ntc_last_error(ctxs[c]));
                        return;
                    }
                }
                // ... and its quality sections (mode keep / bin8), one per block
                std::vector<ntc_qual_meta> qmetas;
                std::shared_ptr<uint8_t> qpl;
                if (q_mode) {
                    uint64_t qn = 0, qbytes = 0;
                    int rq = qh.encode_qualities(ctxs[c], nullptr, 0, nullptr, 0, &qn, &qbytes);
                    if (rq == NTC_ERR_CAPACITY && qn == nblk) {
                        qmetas.resize(qn);
                        qpl.reset((uint8_t *)std::malloc(qbytes ? qbytes : 1), std::free);
                        rq = qpl ? qh.encode_qualities(ctxs[c], qmetas.data(), qn, qpl.get(), qbytes, &qn, &qbytes)
                                 : NTC_ERR_CAPACITY;
                    } else if (rq == NTC_OK || rq == NTC_ERR_CAPACITY) {
                        rq = NTC_ERR_FORMAT;  // (never expected: a section per block)
                    }
                    if (rq) {
                        sh.fail(rq, std::string("encode: qualities: ") + ntc_last_error(ctxs[c]));
                        return;
                    }
                }
                // ... and its name sections (mode keep / id), one per block
                std::vector<ntc_name_meta> nmetas;
                std::shared_ptr<uint8_t> npl;
                if (n_mode) {
                    uint64_t nn = 0, nbytes = 0;
                    int rn = nh.encode_names(ctxs[c], nullptr, 0, nullptr, 0, &nn, &nbytes);
                    if (rn == NTC_ERR_CAPACITY && nn == nblk) {
                        nmetas.resize(nn);
                        npl.reset((uint8_t *)std::malloc(nbytes ? nbytes : 1), std::free);
                        rn = npl ? nh.encode_names(ctxs[c], nmetas.data(), nn, npl.get(), nbytes, &nn, &nbytes)
                                 : NTC_ERR_CAPACITY;
                    } else if (rn == NTC_OK || rn == NTC_ERR_CAPACITY) {
                        rn = NTC_ERR_FORMAT;  // (never expected: a section per block)
                    }
                    if (rn) {
                        sh.fail(rn, std::string("encode: names: ") + ntc_last_error(ctxs[c]));
                        return;
                    }
                }
                // ... and its digests (digests on), one entry per block
                std::vector<ntc_digest_meta> dmetas;
                if (d_mode) {
                    uint64_t dn = 0;
                    int rd = dh.encode_digests(ctxs[c], nullptr, 0, &dn);
                    if (rd == NTC_ERR_CAPACITY && dn == nblk) {
                        dmetas.resize(dn);
                        rd = dh.encode_digests(ctxs[c], dmetas.data(), dn, &dn);
                    } else if (rd == NTC_OK || rd == NTC_ERR_CAPACITY) {
                        rd = NTC_ERR_FORMAT;  // (never expected: an entry per block)
                    }
                    if (rd) {
                        sh.fail(rd, std::string("encode: digests: ") + ntc_last_error(ctxs[c]));
                        return;
                    }
                }
                etrace("gpu done, first block", b.first_block);
                std::lock_guard<std::mutex> g(sh.mu);
                S.gpu_done_s = secs(t0, Clock::now());
                S.bases += b.is_text ? nb : b.offs[b.n_process] - b.offs[0];
                NX.bases += nx_bases;
                if (policy == NTC_NX_MASK) NX.runs += nx_runs;
                b.busy = false;
                size_t run_at = 0;
                for (uint64_t k = 0; k < nblk; k++) {  // streams of the largest payload first
                    const bool ok = metas[k].status == NTC_OK;
                    BlockOut &bo = done[b.first_block + k];
                    bo.status = metas[k].status;
                    bo.n_reads = metas[k].num_records;
                    for (; run_at < runs.size() && runs[run_at].read < (k + 1) * (uint64_t)BR; run_at++) {
                        bo.nx.push_back(runs[run_at]);
                        bo.nx.back().read -= k * (uint64_t)BR;
                    }
                    bo.left = ok ? 4 : 1;
                    if (q_mode && ok) {  // a dropped block takes its section with it
                        bo.has_q = true;
                        bo.qmeta = qmetas[k];
                        bo.left++;
                        tasks.push_back(Task{pl, metas[k], b.first_block + k, 4, qpl});
                    }
                    if (n_mode && ok) {
                        bo.has_n = true;
                        bo.nmeta = nmetas[k];
                        bo.left++;
                        tasks.push_back(Task{pl, metas[k], b.first_block + k, 5, npl});
                    }
                    if (d_mode && ok) {  // (nothing to deflate: the writer puts the 56 bytes out)
                        bo.has_d = true;
                        bo.dmeta = dmetas[k];
                    }
                    int order[4] = {0, 1, 2, 3};
                    std::sort(order, order + 4, [&](int x, int y) {
                        return metas[k].stream[x].encoded_size > metas[k].stream[y].encoded_size;
                    });
                    for (int q = 0; q < (ok ? 4 : 1); q++) tasks.push_back(Task{pl, metas[k], b.first_block + k, order[q]});
                    pending_tasks++;
                }
                sh.cv.notify_all();
            }
        });

    // ---- deflate pool ----------------------------------------------------------------------------
    std::vector<std::thread> pool;
    for (int t = 0; t < T; t++)
        pool.emplace_back([&] {
            for (;;) {
                Task task;
                {
                    std::unique_lock<std::mutex> g(sh.mu);
                    sh.cv.wait(g, [&] { return sh.error != NTC_OK || !tasks.empty(); });
                    if (sh.error != NTC_OK) return;
                    if (tasks.empty()) return;
                    task = std::move(tasks.front());
                    tasks.pop_front();
                }
                uint8_t *data = nullptr;
                uint64_t len = 0;
                const auto td = Clock::now();
                const int status = task.meta.status;
                if (status == NTC_OK && task.stream == 4) {
                    ntc_qual_meta qm;
                    {
                        std::lock_guard<std::mutex> g(sh.mu);
                        qm = done[task.block].qmeta;
                    }
                    const int r = ntc_q_deflate_section(&qm, task.qpayload.get() + qm.payload_off, engine, &data, &len);
                    if (r) {
                        sh.fail(r, "qualities: deflate failed");
                        return;
                    }
                } else if (status == NTC_OK && task.stream == 5) {
                    ntc_name_meta nm;
                    {
                        std::lock_guard<std::mutex> g(sh.mu);
                        nm = done[task.block].nmeta;
                    }
                    const int r = ntc_n_deflate_section(&nm, task.qpayload.get() + nm.payload_off, engine, &data, &len);
                    if (r) {
                        sh.fail(r, "names: deflate failed");
                        return;
                    }
                } else if (status == NTC_OK) {
                    const int r = ntc_deflate_stream(&task.meta, task.stream, task.payload.get(), engine, &data, &len);
                    if (r) {
                        sh.fail(r, "deflate failed");
                        return;
                    }
                } else if (status != NTC_ERR_EMPTY_READ) {
                    sh.fail(status, "malformed block");
                    return;
                }
                task.payload.reset();
                task.qpayload.reset();
                add_time(t_deflate, secs(td, Clock::now()));
                std::lock_guard<std::mutex> g(sh.mu);
                BlockOut &bo = done[task.block];
                if (task.stream == 4) {
                    bo.qsec = data;
                    bo.qlen = len;
                } else if (task.stream == 5) {
                    bo.nsec = data;
                    bo.nlen = len;
                } else {
                    bo.part[task.stream] = data;
                    bo.len[task.stream] = len;
                }
                if (--bo.left == 0) sh.cv.notify_all();
            }
        });

    // ---- writer (this thread) ------------------------------------------------------------------------
    auto write_all = [&](const uint8_t *p, uint64_t n) -> bool {
        while (n) {
            const ssize_t w = ::write(out_fd, p, n);
            if (w <= 0) return false;
            p += w;
            n -= (uint64_t)w;
        }
        return true;
    };
    uint8_t header[32];
    ntc_file_header(header);
    if (!write_all(header, 32)) sh.fail(NTC_ERR_IO, "write failed");
    S.bytes_out = 32;
    // the side file: its header now, then a section per written block that has runs, `read`
    // counted over the reads of the blocks written so far (what decode will print as seq.N - 1)
    if (keep && ntc_nx_write(nx_fd, nullptr, 0, nx_sub, 1)) sh.fail(NTC_ERR_IO, "exceptions: write failed");
    // the quality file: its header, then the section of every block written, in file order
    auto write_q = [&](const uint8_t *p, uint64_t n, int fd) -> bool {
        while (n) {
            const ssize_t w = ::write(fd, p, n);
            if (w < 0 && errno == EINTR) continue;
            if (w <= 0) return false;
            p += w;
            n -= (uint64_t)w;
        }
        return true;
    };
    if (q_mode && ntc_q_write_header2(q_fd, q_mode, q_coder)) sh.fail(NTC_ERR_IO, "qualities: write failed");
    if (n_mode && ntc_n_write_header(n_fd, n_mode)) sh.fail(NTC_ERR_IO, "names: write failed");
    if (d_mode && ntc_d_write_header(d_fd, d_components, d_k, d_nodes)) sh.fail(NTC_ERR_IO, "digests: write failed");
    uint64_t reads_written = 0;
    for (uint64_t blk = 0;; blk++) {
        BlockOut out;
        {
            std::unique_lock<std::mutex> g(sh.mu);
            sh.cv.wait(g, [&] {
                return sh.error != NTC_OK || (done.count(blk) && done[blk].left == 0) ||
                       (reader_done && blk >= total_blocks && !done.count(blk));
            });
            if (sh.error != NTC_OK) break;
            if (!done.count(blk)) break;  // all blocks written
            out = std::move(done[blk]);
            done.erase(blk);
            pending_tasks--;
            writer_at = blk + 1;
            sh.cv.notify_all();
        }
        const auto tw = Clock::now();
        if (out.status == NTC_OK) {
            for (int q = 0; q < 4; q++) {
                if (!write_all(out.part[q], out.len[q])) sh.fail(NTC_ERR_IO, "write failed");
                S.bytes_out += out.len[q];
            }
            S.blocks++;
            if (!out.nx.empty()) {
                uint64_t last_read = UINT64_MAX;
                for (auto &r : out.nx) {
                    NX.reads += r.read != last_read;
                    last_read = r.read;
                    r.read += reads_written;
                }
                if (ntc_nx_write(nx_fd, out.nx.data(), out.nx.size(), nx_sub, 0)) sh.fail(NTC_ERR_IO, "exceptions: write failed");
                NX.runs += out.nx.size();
            }
            reads_written += out.n_reads;
            if (out.has_q) {
                if (!write_q(out.qsec, out.qlen, q_fd)) sh.fail(NTC_ERR_IO, "qualities: write failed");
                QS.sections++;
                QS.quals += out.qmeta.n_quals;
                QS.packed_bytes += out.qmeta.payload_bytes;
                // coder 1 (no gzip member): the section as written
                QS.deflated_bytes += out.qmeta.reserved[0] == 1 ? out.qlen : out.qlen - 24 - out.qmeta.n_syms;
            }
            if (out.has_n) {
                if (!write_q(out.nsec, out.nlen, n_fd)) sh.fail(NTC_ERR_IO, "names: write failed");
                NS.sections++;
                NS.names += out.nmeta.n_reads;
                NS.name_bytes += out.nmeta.name_bytes;
                NS.payload_bytes += out.nmeta.payload_bytes;
                NS.deflated_bytes += out.nlen - 32;
            }
            if (out.has_d) {
                if (const int rd = ntc_d_write_section(d_fd, &out.dmeta))
                    sh.fail(rd == NTC_ERR_IO ? rd : NTC_ERR_FORMAT, "digests: write failed");
                DS.sections++;
                DS.blocks_seq += out.dmeta.components & ntc::kDgSeq ? 1 : 0;
                DS.blocks_sym += out.dmeta.components & ntc::kDgSym ? 1 : 0;
                DS.blocks_qual += out.dmeta.components & ntc::kDgQual ? 1 : 0;
                DS.blocks_name += out.dmeta.components & ntc::kDgName ? 1 : 0;
            }
        } else {
            S.dropped_blocks++;
            NX.runs_in_dropped_blocks += out.nx.size();
        }
        for (int q = 0; q < 4; q++) ntc_buffer_free(out.part[q]);
        ntc_buffer_free(out.qsec);
        ntc_buffer_free(out.nsec);
        add_time(t_write, secs(tw, Clock::now()));
        etrace("written block", blk);
    }
    {
        std::lock_guard<std::mutex> g(sh.mu);
        if (sh.error == NTC_OK) {
            sh.error = -1;  // stop the workers (no more tasks will come)
        }
        sh.cv.notify_all();
    }
    etrace("all written", 0);
    reader.join();
    for (auto &t : gpus) t.join();
    for (auto &t : pool) t.join();
    etrace("threads joined", 0);
    for (auto &kv : done) {
        for (int q = 0; q < 4; q++) ntc_buffer_free(kv.second.part[q]);
        ntc_buffer_free(kv.second.qsec);
        ntc_buffer_free(kv.second.nsec);
    }
    for (auto &b : ring) {
        pinned_free(b.bases);
        pinned_free(b.offs);
        pinned_free(b.text);
    }
    etrace("buffers freed", 0);
    ntc_fastx_close(fx);
    if (fx2) ntc_fastx_close(fx2);
    etrace("input closed", 0);
    const int result = sh.error == -1 ? NTC_OK : sh.error;
    S.alloc_s += t_pin.load();
    S.parse_s = t_parse.load();
    S.gpu_s = t_gpu.load();
    S.deflate_s = t_deflate.load();
    S.write_s = t_write.load();
    S.wall_s = secs(t0, Clock::now());
    S.threads = T;
    S.gpu_parsed = (int32_t)text_batches.load();
    S.bad_read = sh.bad_read;
    std::snprintf(S.error, sizeof(S.error), "%s", result == NTC_OK ? "" : sh.msg.c_str());
    if (stats) *stats = S;
    if (nx) *nx = NX;
    if (qs) *qs = QS;
    if (ns) *ns = NS;
    if (ds) *ds = DS;
    PS.pairs = pair_mode ? S.reads / 2 : 0;
    PS.bytes1 = msrc[0].sent;
    PS.bytes2 = msrc[1].sent;
    if (ps) *ps = PS;
    return result;
}

int ntc_encode_file(ntc_ctx *const *ctxs, int n_ctx, const char *in_path, int out_fd, const ntc_pipeline_opts *opts,
                    ntc_pipeline_stats *stats) {
    return encode_file_impl(ctxs, n_ctx, in_path, out_fd, -1, -1, opts, stats, nullptr);
}

int ntc_encode_file_nx(ntc_ctx *const *ctxs, int n_ctx, const char *in_path, int out_fd, int policy, int nx_fd,
                       const ntc_pipeline_opts *opts, ntc_pipeline_stats *stats, ntc_nx_stats *nx) {
    if (policy < 0) return NTC_ERR_INVALID_ARG;
    return encode_file_impl(ctxs, n_ctx, in_path, out_fd, policy, nx_fd, opts, stats, nx);
}

int ntc_encode_file_ex(ntc_ctx *const *ctxs, int n_ctx, const char *in_path, int out_fd, const ntc_file_opts *fo,
                       const ntc_pipeline_opts *opts, ntc_pipeline_stats *stats, ntc_nx_stats *nx, ntc_q_stats *q) {
    if (!fo || fo->nx_policy < 0) return NTC_ERR_INVALID_ARG;
    return encode_file_impl(ctxs, n_ctx, in_path, out_fd, fo->nx_policy, fo->nx_fd, opts, stats, nx, fo->q_mode,
                            fo->q_fd, q);
}

int ntc_encode_file_ex2(ntc_ctx *const *ctxs, int n_ctx, const char *in_path, int out_fd, const ntc_file_opts2 *fo,
                        const ntc_pipeline_opts *opts, ntc_pipeline_stats *stats, ntc_nx_stats *nx, ntc_q_stats *q,
                        ntc_n_stats *n) {
    if (!fo || fo->struct_bytes < sizeof(ntc_file_opts2) || fo->nx_policy < 0) return NTC_ERR_INVALID_ARG;
    return encode_file_impl(ctxs, n_ctx, in_path, out_fd, fo->nx_policy, fo->nx_fd, opts, stats, nx, fo->q_mode,
                            fo->q_fd, q, fo->n_mode, fo->n_fd, n);
}

int ntc_encode_file_ex3(ntc_ctx *const *ctxs, int n_ctx, const char *in_path, int out_fd, const ntc_file_opts3 *fo,
                        const ntc_pipeline_opts *opts, ntc_pipeline_stats *stats, ntc_nx_stats *nx, ntc_q_stats *q,
                        ntc_n_stats *n, ntc_d_stats *d) {
    if (!fo || fo->struct_bytes < sizeof(ntc_file_opts3) || fo->nx_policy < 0) return NTC_ERR_INVALID_ARG;
    return encode_file_impl(ctxs, n_ctx, in_path, out_fd, fo->nx_policy, fo->nx_fd, opts, stats, nx, fo->q_mode,
                            fo->q_fd, q, fo->n_mode, fo->n_fd, n, fo->d_mode, fo->d_fd, d);
}

int ntc_encode_file_ex4(ntc_ctx *const *ctxs, int n_ctx, const char *in_path, int out_fd, const ntc_file_opts4 *fo,
                        const ntc_pipeline_opts *opts, ntc_pipeline_stats *stats, ntc_nx_stats *nx, ntc_q_stats *q,
                        ntc_n_stats *n, ntc_d_stats *d, ntc_p_stats *p) {
    if (!fo || fo->struct_bytes < sizeof(ntc_file_opts4) || fo->nx_policy < 0) return NTC_ERR_INVALID_ARG;
    return encode_file_impl(ctxs, n_ctx, in_path, out_fd, fo->nx_policy, fo->nx_fd, opts, stats, nx, fo->q_mode,
                            fo->q_fd, q, fo->n_mode, fo->n_fd, n, fo->d_mode, fo->d_fd, d, fo->pair_mode, fo->mate_path, p);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------
// Native decode pipeline of the CLI: `ntcomp decode -i P encoded.dat > out.fasta`
// (src/main.rs:183-211), every stage overlapped:
//
//   extents  the file is mapped; the blocks' extents and record counts come from their
//            32-byte headers alone (block_size of each stream; the flag stream's num_u64 =
//            records).  A truncated block ends the input, as read_exact ends decode_block.
//   unzip    the host pool inflates each block's four streams (ntc_read_block_streams)
//            straight into the batch's pinned payload buffer.
//   GPU      one driver thread per context, batches dealt round-robin:
//            ntc_unpack_streams = H2D of the streams, Rice / minimal-binary decode and
//            zip_block_contents on the device (unpack.hip), the batch's read count back;
//            then, once the reads of the batches before fix its ">seq.N" numbering,
//            ntc_decode_fasta_unpacked = the inverse-SBWT walk, the FASTA text formatted on
//            the GPU, D2H of the text.
//   writer   the calling thread writes the batches' text in file order (a regular file:
//            pwrite at the batch's offset; otherwise write), the next batches' GPU work
//            running meanwhile.  Batches are numbered by whichever thread completes a read
//            count.
// NTC_HOST_UNPACK=1: the pool decodes each block into u64 records (ntc_read_block_into),
// counting its reads, and ntc_decode_fasta takes the records.
// A damaged block ends the output after the blocks before it (decode_block's Err ends the
// reference's loop, main.rs:202).
// ---------------------------------------------------------------------------------------
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>

namespace {

struct DBlock {
    uint64_t a, len;   // byte range of the block
    uint64_t n_recs;   // records (the flag stream's num_u64)
    uint64_t pay;      // bytes of its four inflated streams (8 x encoded_size each)
    bool bad;          // a header that cannot describe its gzip stream: damaged, never sized
};

struct DSlot {  // one batch in flight
    uint64_t *recs = nullptr;
    uint64_t cap_recs = 0;
    uint8_t *pay = nullptr;  // GPU unpack: the blocks' inflated streams
    uint64_t cap_pay = 0, n_pay = 0;
    std::vector<ntc_block_meta> metas;
    uint8_t *text = nullptr;
    uint64_t cap_text = 0;
    uint64_t batch = ~0ULL;  // batch held, ~0 = free
    uint64_t first_block = 0, n_blocks = 0;
    uint64_t n_recs = 0, n_reads = 0, n_bases = 0, text_len = 0;
    uint64_t first_len = 0;  // pairs: the bytes of the mate-1 part, at the head of text
    uint64_t first_id = 0;
    uint64_t finished = 0;   // blocks of this batch unzipped or found damaged
    int bad_block = -1;      // first damaged block (index in the batch)
    bool buffer = false;     // recs sized for the batch
    bool ready = false;      // complete + first_id known: the GPU may take it
    bool unpacked = false;   // GPU unpack: the batch's reads and bases are known
    bool decoded = false;
};

void count_reads(const uint64_t *r, uint64_t n, uint64_t *reads, uint64_t *bases) {
    uint64_t rd = 0, bs = 0;  // first flags and bases of records (flag byte = bits 56..63)
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t w = r[i];
        const uint32_t flag = (uint32_t)(w >> 56);
        rd += flag & 1;
        bs += (flag & 2) ? (flag >> 2) : ((w >> 32) & 0xFFFFFFu);
    }
    *reads += rd;
    *bases += bs;
}

uint64_t digits_total(uint64_t first, uint64_t n) {  // decimal digits of first .. first + n - 1
    uint64_t tot = 0;
    for (uint64_t lo = 1, d = 1; n && lo <= first + n - 1; lo *= 10, d++) {
        const uint64_t hi = lo > UINT64_MAX / 10 ? UINT64_MAX : lo * 10 - 1;
        const uint64_t a = std::max(lo, first), b = std::min(hi, first + n - 1);
        if (a <= b) tot += d * (b - a + 1);
        if (hi == UINT64_MAX) break;
    }
    return tot;
}

}  // namespace

extern "C" {

// nx_path: ntc_decode_file_nx's side file (null: none)
// q_path: ntc_decode_file_ex's quality file (null: none; the output is then FASTA)
static int decode_file_impl(ntc_ctx *const *ctxs, int n_ctx, const char *in_path, const char *nx_path, int out_fd,
                            const ntc_pipeline_opts *opts, ntc_pipeline_stats *stats, const char *q_path = nullptr,
                            const char *n_path = nullptr, const char *d_path = nullptr, ntc_d_stats *ds = nullptr,
                            bool may_discard = false, int pair_mode = 0, int out_fd2 = -1, ntc_p_stats *ps = nullptr) {
    // d_path / ds: ntc_decode_file_ex3's digest file (null: none); may_discard: out_fd -1 runs
    // everything but the copy of the text off the device and its write
    const bool discard = may_discard && out_fd == -1;
    if (!ctxs || n_ctx <= 0 || !in_path || (out_fd < 0 && !discard)) return NTC_ERR_INVALID_ARG;
    // pair_mode / out_fd2 / ps: ntc_decode_file_ex4's pairs (pair_mode 0: none): each batch's text
    // comes back split, its mate-1 records go to out_fd and its mate-2 records to out_fd2
    if (pair_mode < 0 || pair_mode > 2 || (pair_mode ? out_fd2 < 0 && !discard : out_fd2 != -1)) return NTC_ERR_INVALID_ARG;
    const ntc::PHooks &ph = ntc::g_p_hooks;
    if (pair_mode && (!ph.set_mode || !ph.pair_split)) return NTC_ERR_UNSUPPORTED;
    const bool split = pair_mode && !discard;
    ntc_p_stats PS{};
    PS.mode = (uint32_t)pair_mode;
    for (int i = 0; i < n_ctx; i++)
        if (!ctxs[i]) return NTC_ERR_INVALID_ARG;
    // the exception runs, read once; each batch finds its own by its first read (put_runs)
    struct NxFile {
        ntc_nx_run *runs = nullptr;
        uint64_t n = 0;
        uint32_t sub = 0;
        ~NxFile() { ntc_buffer_free(runs); }
    } nxf;
    if (nx_path) {
        if (!ntc::g_nx_hooks.decode_set_exceptions) return NTC_ERR_UNSUPPORTED;
        if (const int r = ntc_nx_read(nx_path, &nxf.runs, &nxf.n, &nxf.sub)) {
            if (stats) {
                std::memset(stats, 0, sizeof(*stats));
                stats->bad_read = -1;
                std::snprintf(stats->error, sizeof(stats->error), "exceptions: %s",
                              r == NTC_ERR_IO ? "cannot read the side file" : "malformed side file");
            }
            return r;
        }
    }
    // the quality sections, read once; section i belongs to block i of the file
    struct QFile {
        ntc_qual_meta *metas = nullptr;
        uint64_t n = 0, bytes = 0;
        uint8_t *payload = nullptr;
        int mode = 0;
        ~QFile() {
            ntc_buffer_free(metas);
            ntc_buffer_free(payload);
        }
    } qf;
    if (q_path) {
        if (!ntc::g_q_hooks.decode_set_qualities) return NTC_ERR_UNSUPPORTED;
        if (const int r = ntc_q_read(q_path, &qf.mode, &qf.metas, &qf.n, &qf.payload, &qf.bytes)) {
            if (stats) {
                std::memset(stats, 0, sizeof(*stats));
                stats->bad_read = -1;
                std::snprintf(stats->error, sizeof(stats->error), "qualities: %s",
                              r == NTC_ERR_IO ? "cannot read the side file" : "malformed side file");
            }
            return r;
        }
    }
    // hands ctx the sections of blocks [first, first + n), their words from offset 0
    auto put_quals = [&](ntc_ctx *ctx, uint64_t first, uint64_t n, std::vector<ntc_qual_meta> &tmp) -> int {
        if (!q_path || n == 0) return NTC_OK;
        if (first + n > qf.n) return NTC_ERR_FORMAT;
        tmp.assign(qf.metas + first, qf.metas + first + n);
        const uint64_t base = tmp[0].payload_off;
        for (auto &m : tmp) m.payload_off -= base;
        const uint64_t bytes = tmp.back().payload_off + tmp.back().payload_bytes;
        return ntc::g_q_hooks.decode_set_qualities(ctx, tmp.data(), n, qf.payload + base, bytes);
    };
    // the name sections, likewise
    struct NFile {
        ntc_name_meta *metas = nullptr;
        uint64_t n = 0, bytes = 0;
        uint8_t *payload = nullptr;
        int mode = 0;
        ~NFile() {
            ntc_buffer_free(metas);
            ntc_buffer_free(payload);
        }
    } nf;
    if (n_path) {
        if (!ntc::g_n_hooks.decode_set_names) return NTC_ERR_UNSUPPORTED;
        if (const int r = ntc_n_read(n_path, &nf.mode, &nf.metas, &nf.n, &nf.payload, &nf.bytes)) {
            if (stats) {
                std::memset(stats, 0, sizeof(*stats));
                stats->bad_read = -1;
                std::snprintf(stats->error, sizeof(stats->error), "names: %s",
                              r == NTC_ERR_IO ? "cannot read the side file" : "malformed side file");
            }
            return r;
        }
    }
    // hands ctx the name sections of blocks [first, first + n); *bytes = their names' bytes
    auto put_names = [&](ntc_ctx *ctx, uint64_t first, uint64_t n, std::vector<ntc_name_meta> &tmp) -> int {
        if (!n_path || n == 0) return NTC_OK;
        if (first + n > nf.n) return NTC_ERR_FORMAT;
        tmp.assign(nf.metas + first, nf.metas + first + n);
        const uint64_t base = tmp[0].payload_off;
        for (auto &m : tmp) m.payload_off -= base;
        const uint64_t bytes = tmp.back().payload_off + tmp.back().payload_bytes;
        return ntc::g_n_hooks.decode_set_names(ctx, tmp.data(), n, nf.payload + base, bytes);
    };
    // the expected digests, likewise; the file names the index it was written against
    struct DFile {
        ntc_digest_meta *metas = nullptr;
        uint64_t n = 0, n_nodes = 0;
        uint32_t components = 0, k = 0;
        ~DFile() { ntc_buffer_free(metas); }
    } df;
    ntc_d_stats DS{};
    const ntc::DHooks &dh = ntc::g_d_hooks;
    if (discard && !dh.set_discard) return NTC_ERR_UNSUPPORTED;
    if (d_path) {
        if (!dh.decode_set_digests || !dh.decode_digests || !dh.index_info) return NTC_ERR_UNSUPPORTED;
        int r = ntc_d_read(d_path, &df.components, &df.k, &df.n_nodes, &df.metas, &df.n);
        char why[200];
        std::snprintf(why, sizeof(why), "digests: %s", r == NTC_ERR_IO ? "cannot read the side file" : "malformed side file");
        uint64_t nodes = 0;
        uint32_t k = 0;
        if (!r && (r = dh.index_info(ctxs[0], &nodes, &k))) std::snprintf(why, sizeof(why), "digests: no index uploaded");
        if (!r && (k != df.k || nodes != df.n_nodes)) {
            r = NTC_ERR_DIGEST;
            std::snprintf(why, sizeof(why), "digests: the file was written against another index (k = %u, %llu nodes; "
                          "the index uploaded has k = %u, %llu nodes)", df.k, (unsigned long long)df.n_nodes, k,
                          (unsigned long long)nodes);
        }
        if (r) {
            if (stats) {
                std::memset(stats, 0, sizeof(*stats));
                stats->bad_read = -1;
                std::snprintf(stats->error, sizeof(stats->error), "%s", why);
            }
            return r;
        }
    }
    // hands ctx the expected digests of blocks [first, first + n)
    auto put_digests = [&](ntc_ctx *ctx, uint64_t first, uint64_t n) -> int {
        if (!d_path) return NTC_OK;
        if (first + n > df.n) return NTC_ERR_FORMAT;
        return dh.decode_set_digests(ctx, df.metas + first, n);
    };
    // after a batch's decode call (rc): what it checked into the stats (under sh.mu), and for
    // NTC_ERR_DIGEST the block in the file's numbering, its first read and the component
    auto digest_verdict = [&](ntc_ctx *ctx, int rc, uint64_t first, uint64_t n, uint64_t first_read, std::string &msg,
                              int64_t &bad_read) {
        if (!d_path || n == 0 || (rc != NTC_OK && rc != NTC_ERR_DIGEST)) return;
        std::vector<ntc_digest_meta> got(n);
        uint64_t have = 0;
        if (dh.decode_digests(ctx, got.data(), n, &have) != NTC_OK || have != n) return;
        static const char *const names[4] = {"seq", "sym", "qual", "name"};
        uint64_t read = first_read;
        for (uint64_t b = 0; b < n; b++) {
            const ntc_digest_meta &e = df.metas[first + b], &g = got[b];
            const uint64_t ed[4] = {e.d_seq, e.d_sym, e.d_qual, e.d_name}, gd[4] = {g.d_seq, g.d_sym, g.d_qual, g.d_name};
            if (rc == NTC_ERR_DIGEST) {
                int at = g.n_bases != e.n_bases ? 0 : -1;
                for (int c = 0; c < 4 && at < 0; c++)
                    if ((g.components >> c & 1) && ed[c] != gd[c]) at = c;
                if (at >= 0) {
                    char buf[240];
                    std::snprintf(buf, sizeof(buf), "digest mismatch in block %llu (first read %llu), component %s: expected "
                                  "0x%016llx, computed 0x%016llx", (unsigned long long)(first + b), (unsigned long long)read,
                                  names[at], (unsigned long long)ed[at], (unsigned long long)gd[at]);
                    msg = buf;
                    bad_read = (int64_t)read;
                    return;
                }
            } else {
                DS.sections++;
                DS.blocks_seq += g.components & ntc::kDgSeq ? 1 : 0;
                DS.blocks_sym += g.components & ntc::kDgSym ? 1 : 0;
                DS.blocks_qual += g.components & ntc::kDgQual ? 1 : 0;
                DS.blocks_name += g.components & ntc::kDgName ? 1 : 0;
                DS.not_checkable |= e.components & ~g.components;
            }
            read += e.n_reads;
        }
    };
    // the names' bytes of blocks [first, first + n) (those the side file has): room in the text
    auto name_room = [&](uint64_t first, uint64_t n) -> uint64_t {
        uint64_t bytes = 0;
        for (uint64_t k = first; n_path && k < first + n && k < nf.n; k++) bytes += nf.metas[k].name_bytes;
        return bytes;
    };
    const uint64_t q_per_base = q_path ? 1 : 0, q_per_read = q_path ? 3 : 0;  // FASTQ: "+\n", qualities, "\n" more
    // hands ctx the runs of reads [first, first + n) (file numbering), read relative to first
    auto put_runs = [&](ntc_ctx *ctx, uint64_t first, uint64_t n, std::vector<ntc_nx_run> &tmp) -> int {
        if (!nxf.n) return NTC_OK;
        const auto less = [](const ntc_nx_run &x, uint64_t v) { return x.read < v; };
        const ntc_nx_run *lo = std::lower_bound(nxf.runs, nxf.runs + nxf.n, first, less);
        const ntc_nx_run *hi = std::lower_bound(lo, (const ntc_nx_run *)(nxf.runs + nxf.n), first + n, less);
        tmp.assign(lo, hi);
        for (auto &r : tmp) r.read -= first;
        return ntc::g_nx_hooks.decode_set_exceptions(ctx, tmp.data(), tmp.size(), nxf.sub);
    };
    ntc_pipeline_opts o{};
    if (opts) o = *opts;
    const int T = o.threads > 0 ? o.threads : ntc_host_threads();
    // two blocks per GPU call: ~21 MB of text per batch keeps the pinned ring small and the
    // writer (the bound: ~8 GB/s into one file's page cache) busy from the first 20 ms
    const uint64_t bpb = (uint64_t)(o.blocks_per_batch > 0 ? o.blocks_per_batch : 2);
    ntc_pipeline_stats S{};
    const auto t0 = Clock::now();

    // ---- map + extents ------------------------------------------------------------------
    const int fd = ::open(in_path, O_RDONLY);
    if (fd < 0) return NTC_ERR_IO;
    struct stat st;
    if (fstat(fd, &st) != 0) {
        ::close(fd);
        return NTC_ERR_IO;
    }
    const uint64_t fsize = (uint64_t)st.st_size;
    const uint8_t *data = nullptr;
    if (fsize) {
        data = (const uint8_t *)mmap(nullptr, fsize, PROT_READ, MAP_PRIVATE, fd, 0);
        if (data == MAP_FAILED) {
            ::close(fd);
            return NTC_ERR_IO;
        }
        madvise((void *)data, fsize, MADV_SEQUENTIAL);
    }
    ::close(fd);
    auto le32 = [&](uint64_t p) { return (uint64_t)data[p] | (uint64_t)data[p + 1] << 8 | (uint64_t)data[p + 2] << 16 |
                                         (uint64_t)data[p + 3] << 24; };
    // A block's buffers are sized from its headers before anything is inflated, so each
    // header is checked against its own gzip stream first: the ISIZE trailer must equal
    // 8 x encoded_size, which deflate cannot exceed 1032 x block_size, and stream 2 (Rice: one
    // bit per value at least) bounds num_u64.  A block that fails is damaged -- the output ends
    // before it, as the reference's loop ends at decode_block's Err (main.rs:202) -- instead of
    // a pinned allocation sized from garbage.
    std::vector<DBlock> blocks;
    for (uint64_t pos = 32; pos < fsize;) {  // after the 32-byte file header (main.rs:196-198)
        uint64_t p = pos, nrec = 0, pay = 0;
        bool whole = true, bad = false;
        for (int s = 0; s < 4 && whole; s++) {
            if (p + 32 > fsize) {
                whole = false;
                break;
            }
            const uint64_t bs = le32(p), enc = le32(p + 12);
            if (s == 2) nrec = le32(p + 8);
            if (bs < 18 || p + 32 + bs > fsize || le32(p + 32 + bs - 4) != ((8 * enc) & 0xFFFFFFFFULL) ||
                8 * enc > 1032 * bs || (s == 2 && nrec > 64 * enc))
                bad = true;
            pay += 8 * enc;
            p += 32 + bs;
            if (p > fsize) whole = false;
        }
        if (!whole) break;
        // a bad block is sized as nothing; the unzip pool reports it damaged
        blocks.push_back(bad ? DBlock{pos, p - pos, 0, 0, true} : DBlock{pos, p - pos, nrec, pay, false});
        pos = p;
    }
    // NTC_FIRST_BATCH_BLOCKS=n: batch 0 holds n blocks, the others blocks_per_batch.  A
    // one-block first batch (the writer -- the pipeline's bound -- starting sooner) measured
    // no better on the box: the first write still came at ~20 ms, pipeline 0.160-0.198 s
    // against 0.166-0.178 s (profiles/round6/e2e_first_batch/), so the default stays bpb.
    const char *fbe = std::getenv("NTC_FIRST_BATCH_BLOCKS");
    const uint64_t b0n = std::max<uint64_t>(1, std::min<uint64_t>(bpb, fbe ? (uint64_t)std::atoll(fbe) : bpb));
    auto batch_first = [&](uint64_t b) -> uint64_t { return b == 0 ? 0 : b0n + (b - 1) * bpb; };
    auto batch_of = [&](uint64_t blk) -> uint64_t { return blk < b0n ? 0 : 1 + (blk - b0n) / bpb; };
    auto batch_end = [&](uint64_t b) -> uint64_t { return std::min<uint64_t>(blocks.size(), batch_first(b + 1)); };
    const uint64_t n_batches = blocks.empty() ? 0 : batch_of(blocks.size() - 1) + 1;
    S.alloc_s = secs(t0, Clock::now());

    const int NB = n_ctx + 2;
    std::vector<DSlot> slots((size_t)NB);
    // the streams decoded on the GPU (default) or on the host pool (NTC_HOST_UNPACK=1): the
    // 10 M-read decode pipeline ran at 8.0 against 7.6 Gbases/s on one MI355X box, the pool's
    // thread-time 0.11 against 0.64 s (profiles/round5/e2e_dec_*)
    const bool gpu_unpack = !host_unpack_on();
    // NTC_PIPE_TRACE=n: the first n batches' events on stderr (ms from the call's start)
    const char *tr = std::getenv("NTC_PIPE_TRACE");
    const uint64_t trace_n = tr ? (uint64_t)std::atoll(tr) : 0;
    auto trace = [&](const char *what, uint64_t b) {
        if (b < trace_n) std::fprintf(stderr, "[pipe] %8.3f ms batch %llu %s\n", 1e3 * secs(t0, Clock::now()),
                                      (unsigned long long)b, what);
    };
    Shared sh;
    uint64_t next_task = 0;       // next block to unzip
    uint64_t next_id = 1;         // main.rs:204: seq.{i+1}
    int64_t stop_batch = -1;      // batch holding the first damaged block (output ends in it)
    std::atomic<double> t_unzip{0}, t_gpu{0}, t_write{0}, t_pin{0};
    auto add_time = [](std::atomic<double> &a, double d) {
        double cur = a.load();
        while (!a.compare_exchange_weak(cur, cur + d)) {
        }
    };
    auto slot_of = [&](uint64_t b) -> DSlot & { return slots[(size_t)(b % (uint64_t)NB)]; };
    // pinned buffers are sized per batch (grown in the claiming thread, outside the lock)
    auto ensure_pinned = [&](void **p, uint64_t *cap, uint64_t need) -> bool {
        if (need <= *cap) return true;
        const auto tp = Clock::now();
        struct Acc {
            std::atomic<double> &a;
            Clock::time_point t;
            ~Acc() {
                double cur = a.load(), d = secs(t, Clock::now());
                while (!a.compare_exchange_weak(cur, cur + d)) {
                }
            }
        } acc{t_pin, tp};
        pinned_free(*p);
        *p = nullptr;
        *cap = 0;
        const uint64_t want = need + need / 8 + 4096;
        if (!(*p = pinned_alloc(want))) return false;
        *cap = want;
        return true;
    };

    // ">seq.N" numbering: batch a gets first_id once every batch before it has its read count
    // (host unpack: the batch is complete; GPU unpack: the device has decoded its streams).
    // Whichever thread completes a count numbers the batches as far ahead as they allow, so
    // their GPU work overlaps the writes of the batches before them (round 5's first version
    // numbered them in the writer's loop only: a batch's text then waited for the write of
    // the one before it, 3.1 ms per batch where the write takes 2).
    uint64_t next_assign = 0;
    auto assign_ahead = [&]() {  // under sh.mu
        while (next_assign < n_batches) {
            if (stop_batch >= 0 && (int64_t)next_assign > stop_batch) break;
            DSlot &sl = slot_of(next_assign);
            if (sl.batch != next_assign || sl.finished != sl.n_blocks) break;
            if (gpu_unpack && !sl.unpacked) break;
            if (!gpu_unpack && sl.bad_block >= 0) {  // only the blocks before the damaged one
                uint64_t n = 0;
                for (int i = 0; i < sl.bad_block; i++) n += blocks[sl.first_block + (uint64_t)i].n_recs;
                sl.n_recs = n;
                sl.n_reads = sl.n_bases = 0;
                count_reads(sl.recs, n, &sl.n_reads, &sl.n_bases);
            }
            sl.first_id = next_id;
            next_id += sl.n_reads;
            sl.ready = true;
            next_assign++;
            sh.cv.notify_all();
        }
    };
    // ---- GPU drivers ---------------------------------------------------------------------------
    // A batch is complete when all of its blocks are in (or every block before its first
    // damaged one, once no task of it is still running).  The assigner (below, in the
    // writer's loop) fixes first_id in batch order.
    std::vector<std::thread> gpus;
    for (int c = 0; c < n_ctx; c++)
        gpus.emplace_back([&, c] {
            // While the pool inflates the first batches: one tiny unpack (an empty block) and
            // one tiny decode (a one-base read), so the first real calls find the unpacker's
            // and the formatter's code objects loaded (HIP loads them at a kernel's first
            // launch: ~10 ms on the first batch's path otherwise)
            if (gpu_unpack && !std::getenv("NTC_NO_WARM")) {
                ntc_block_meta m0{};
                uint64_t ok = 0, nr = 0, nbs = 0, len = 0, brecs = 0, bpay = 0;
                uint8_t pay0[8] = {0}, txt[64];
                const uint64_t rec1 = (uint64_t)(1u | 2u | (1u << 2)) << 56;  // first, short, 1 base "A"
                // (the larger of this context's first two batches: batch 0 is one block)
                for (uint64_t b2 = (uint64_t)c; b2 < n_batches && b2 <= (uint64_t)c + (uint64_t)n_ctx; b2 += (uint64_t)n_ctx) {
                    uint64_t r2 = 0, p2 = 0;
                    for (uint64_t i = batch_first(b2); i < batch_end(b2); i++) {
                        r2 += blocks[i].n_recs;
                        p2 += blocks[i].pay;
                    }
                    brecs = std::max(brecs, r2);
                    bpay = std::max(bpay, p2);
                }
                // ... and the device workspaces sized for the first batches (hipMalloc'd here)
                trace("warm-up start", c);
                const int w1 = ntc_unpack_streams(ctxs[c], pay0, 8, &m0, 1, &ok, &nr, &nbs);
                trace("warm-up unpack", c);
                const int w2 = w1 ? w1 : ntc_decode_fasta(ctxs[c], &rec1, 1, 1, 1, 1, txt, sizeof(txt), &len);
                trace("warm-up decode", c);
                const int w3 = w2 ? w2 : ntc::reserve_decode(ctxs[c], bpay, brecs, nullptr, 0);
                trace("warm-up reserve", c);
                if (w3) {
                    sh.fail(NTC_ERR_HIP, std::string("decode: ") + ntc_last_error(ctxs[c]));
                    return;
                }
            }
            // out_fd -1: the text stays on the device (the context drops the option when this thread ends)
            struct Discard {
                ntc_ctx *ctx;
                ~Discard() {
                    if (ctx) ntc::g_d_hooks.set_discard(ctx, 0);
                }
            } discard_reset{discard ? ctxs[c] : nullptr};
            if (discard && dh.set_discard(ctxs[c], 1)) {
                sh.fail(NTC_ERR_HIP, std::string("decode: ") + ntc_last_error(ctxs[c]));
                return;
            }
            // pairs: every text call of this thread returns its two parts (option dropped at its end)
            struct Pairs {
                ntc_ctx *ctx;
                ~Pairs() {
                    if (ctx) ntc::g_p_hooks.set_mode(ctx, 0);
                }
            } pairs_reset{split ? ctxs[c] : nullptr};
            if (split && ph.set_mode(ctxs[c], pair_mode)) {
                sh.fail(NTC_ERR_HIP, std::string("decode: ") + ntc_last_error(ctxs[c]));
                return;
            }
            std::vector<ntc_nx_run> nx_tmp;  // a batch's exception runs, renumbered from its first read
            std::vector<ntc_qual_meta> q_tmp;  // ... and its quality sections
            std::vector<ntc_name_meta> n_tmp;  // ... and its name sections
            for (uint64_t b = (uint64_t)c;; b += (uint64_t)n_ctx) {
                DSlot *slp;
                if (gpu_unpack) {
                    // the batch's streams decoded on the device as soon as every block of it is
                    // inflated (or found damaged): its read count numbers the batches after it
                    {
                        std::unique_lock<std::mutex> g(sh.mu);
                        sh.cv.wait(g, [&] {
                            return sh.error != NTC_OK || b >= n_batches || (stop_batch >= 0 && (int64_t)b > stop_batch) ||
                                   (slot_of(b).batch == b && slot_of(b).finished == slot_of(b).n_blocks);
                        });
                        if (sh.error != NTC_OK || b >= n_batches || (stop_batch >= 0 && (int64_t)b > stop_batch)) return;
                        slp = &slot_of(b);
                    }
                    DSlot &sl = *slp;
                    const uint64_t nb = sl.bad_block >= 0 ? (uint64_t)sl.bad_block : sl.n_blocks;
                    const auto tg = Clock::now();
                    uint64_t ok = 0, nr = 0, nbs = 0;
                    const int rc = ntc_unpack_streams(ctxs[c], sl.pay, sl.n_pay, sl.metas.data(), nb, &ok, &nr, &nbs);
                    add_time(t_gpu, secs(tg, Clock::now()));
                    if (rc) {
                        sh.fail(rc, std::string("decode: ") + ntc_last_error(ctxs[c]));
                        return;
                    }
                    {
                        std::unique_lock<std::mutex> g(sh.mu);
                        if (ok < nb) {  // a block the device could not decode: the output ends before it
                            sl.bad_block = (int)ok;
                            if (stop_batch < 0 || (int64_t)b < stop_batch) stop_batch = (int64_t)b;
                        }
                        sl.n_reads = nr;
                        sl.n_bases = nbs;
                        sl.unpacked = true;
                        trace("unpacked", b);
                        assign_ahead();
                        sh.cv.notify_all();
                        sh.cv.wait(g, [&] { return sh.error != NTC_OK || sl.ready; });
                        if (sh.error != NTC_OK) return;
                    }
                    const uint64_t need = sl.n_bases * (1 + q_per_base) + (7 + q_per_read) * sl.n_reads +
                                          digits_total(sl.first_id, sl.n_reads) + name_room(sl.first_block, nb) + 64;
                    const auto tf = Clock::now();
                    if (!discard && !ensure_pinned((void **)&sl.text, &sl.cap_text, need)) {
                        sh.fail(NTC_ERR_HIP, "pinned host allocation failed");
                        return;
                    }
                    uint64_t len = 0;
                    if (const int rx = put_runs(ctxs[c], sl.first_id - 1, sl.n_reads, nx_tmp)) {
                        sh.fail(rx, std::string("decode: ") + ntc_last_error(ctxs[c]));
                        return;
                    }
                    if (const int rx = put_quals(ctxs[c], sl.first_block, nb, q_tmp)) {
                        sh.fail(rx, rx == NTC_ERR_FORMAT ? "qualities: fewer sections than blocks, or a section that "
                                                           "does not fit its block"
                                                         : std::string("decode: ") + ntc_last_error(ctxs[c]));
                        return;
                    }
                    if (const int rx = put_names(ctxs[c], sl.first_block, nb, n_tmp)) {
                        sh.fail(rx, rx == NTC_ERR_FORMAT ? "names: fewer sections than blocks, or a section that does "
                                                           "not fit its block"
                                                         : std::string("decode: ") + ntc_last_error(ctxs[c]));
                        return;
                    }
                    if (const int rx = put_digests(ctxs[c], sl.first_block, nb)) {
                        sh.fail(rx, rx == NTC_ERR_FORMAT ? "digests: fewer sections than blocks"
                                                         : std::string("decode: ") + ntc_last_error(ctxs[c]));
                        return;
                    }
                    const int rf = ntc_decode_fasta_unpacked(ctxs[c], sl.first_id, sl.text, discard ? 0 : sl.cap_text, &len);
                    add_time(t_gpu, secs(tf, Clock::now()));
                    if (rf) {
                        std::string msg = std::string("decode: ") + ntc_last_error(ctxs[c]);
                        int64_t bad = -1;
                        digest_verdict(ctxs[c], rf, sl.first_block, nb, sl.first_id - 1, msg, bad);
                        sh.fail(rf, msg, bad);
                        return;
                    }
                    uint64_t first = 0;
                    if (split && ph.pair_split(ctxs[c], &first)) {
                        sh.fail(NTC_ERR_FORMAT, std::string("decode: ") + ntc_last_error(ctxs[c]));
                        return;
                    }
                    std::lock_guard<std::mutex> g(sh.mu);
                    {
                        std::string unused;
                        int64_t bad = -1;
                        digest_verdict(ctxs[c], NTC_OK, sl.first_block, nb, sl.first_id - 1, unused, bad);
                    }
                    sl.first_len = first;
                    sl.text_len = len;
                    sl.decoded = true;
                    trace("decoded", b);
                    S.gpu_done_s = secs(t0, Clock::now());
                    sh.cv.notify_all();
                    continue;
                }
                {
                    std::unique_lock<std::mutex> g(sh.mu);
                    sh.cv.wait(g, [&] {
                        return sh.error != NTC_OK || b >= n_batches || (stop_batch >= 0 && (int64_t)b > stop_batch) ||
                               (slot_of(b).batch == b && slot_of(b).ready);
                    });
                    if (sh.error != NTC_OK || b >= n_batches || (stop_batch >= 0 && (int64_t)b > stop_batch)) return;
                    slp = &slot_of(b);
                }
                DSlot &sl = *slp;
                const uint64_t nrec = sl.n_recs;
                const uint64_t need = sl.n_bases * (1 + q_per_base) + (7 + q_per_read) * sl.n_reads +
                                      digits_total(sl.first_id, sl.n_reads) + name_room(sl.first_block, sl.n_blocks) + 64;
                const auto tg = Clock::now();
                if (!discard && !ensure_pinned((void **)&sl.text, &sl.cap_text, need)) {
                    sh.fail(NTC_ERR_HIP, "pinned host allocation failed");
                    return;
                }
                uint64_t len = 0;
                if (const int rx = put_runs(ctxs[c], sl.first_id - 1, sl.n_reads, nx_tmp)) {
                    sh.fail(rx, std::string("decode: ") + ntc_last_error(ctxs[c]));
                    return;
                }
                if (const int rx = put_quals(ctxs[c], sl.first_block,
                                             sl.bad_block >= 0 ? (uint64_t)sl.bad_block : sl.n_blocks, q_tmp)) {
                    sh.fail(rx, rx == NTC_ERR_FORMAT ? "qualities: fewer sections than blocks, or a section that "
                                                       "does not fit its block"
                                                     : std::string("decode: ") + ntc_last_error(ctxs[c]));
                    return;
                }
                if (const int rx = put_names(ctxs[c], sl.first_block,
                                             sl.bad_block >= 0 ? (uint64_t)sl.bad_block : sl.n_blocks, n_tmp)) {
                    sh.fail(rx, rx == NTC_ERR_FORMAT ? "names: fewer sections than blocks, or a section that does "
                                                       "not fit its block"
                                                     : std::string("decode: ") + ntc_last_error(ctxs[c]));
                    return;
                }
                const uint64_t nbk = sl.bad_block >= 0 ? (uint64_t)sl.bad_block : sl.n_blocks;
                if (const int rx = put_digests(ctxs[c], sl.first_block, nbk)) {
                    sh.fail(rx, rx == NTC_ERR_FORMAT ? "digests: fewer sections than blocks"
                                                     : std::string("decode: ") + ntc_last_error(ctxs[c]));
                    return;
                }
                const int rc = ntc_decode_fasta(ctxs[c], sl.recs, nrec, sl.n_reads, sl.n_bases, sl.first_id, sl.text,
                                                discard ? 0 : sl.cap_text, &len);
                add_time(t_gpu, secs(tg, Clock::now()));
                if (rc) {
                    std::string msg = std::string("decode: ") + ntc_last_error(ctxs[c]);
                    int64_t bad = -1;
                    digest_verdict(ctxs[c], rc, sl.first_block, nbk, sl.first_id - 1, msg, bad);
                    sh.fail(rc, msg, bad);
                    return;
                }
                uint64_t first = 0;
                if (split && ph.pair_split(ctxs[c], &first)) {
                    sh.fail(NTC_ERR_FORMAT, std::string("decode: ") + ntc_last_error(ctxs[c]));
                    return;
                }
                std::lock_guard<std::mutex> g(sh.mu);
                {
                    std::string unused;
                    int64_t bad = -1;
                    digest_verdict(ctxs[c], NTC_OK, sl.first_block, nbk, sl.first_id - 1, unused, bad);
                }
                sl.first_len = first;
                sl.text_len = len;
                sl.decoded = true;
                trace("decoded", b);
                S.gpu_done_s = secs(t0, Clock::now());
                sh.cv.notify_all();
            }
        });

    // ---- pinned buffers of the first batches, allocated in parallel -----------------------------
    // (each is mapped, touched and registered: ~10 ms for a batch's 21 MB of text, which the
    // first batch would otherwise wait for in turn; later batches reuse them).  The text size
    // is a guess from the records (48 bytes each: C91's reads take 41); a batch that needs
    // more regrows its buffer as before.
    {
        std::vector<std::thread> pre;
        for (uint64_t j = 0; j < (uint64_t)NB && j < n_batches; j++)
            pre.emplace_back([&, j] {
                uint64_t nr = 0, np = 0;
                for (uint64_t i = batch_first(j); i < batch_end(j); i++) {
                    nr += blocks[i].n_recs;
                    np += blocks[i].pay;
                }
                DSlot &sl = slots[(size_t)j];
                const bool ok = (gpu_unpack ? ensure_pinned((void **)&sl.pay, &sl.cap_pay, np + 8)
                                            : ensure_pinned((void **)&sl.recs, &sl.cap_recs, nr * 8 + 8)) &&
                                (discard || ensure_pinned((void **)&sl.text, &sl.cap_text, nr * 48 + (1u << 20)));
                if (!ok) sh.fail(NTC_ERR_HIP, "pinned host allocation failed");
            });
        for (auto &t : pre) t.join();
    }

    // ---- unzip pool ------------------------------------------------------------------------
    // Blocks are taken in file order; the first block of a batch claims the batch's slot
    // (free once the writer is done with batch b - NB) and sizes its record buffer.  Past a
    // damaged block no later batch is started; the rest of its own batch is still unzipped
    // so that the batch completes (only the blocks before the damaged one are decoded).
    std::vector<std::thread> pool;
    for (int t = 0; t < T; t++)
        pool.emplace_back([&] {
            for (;;) {
                uint64_t blk, b;
                bool first;
                {
                    std::unique_lock<std::mutex> g(sh.mu);
                    auto exhausted = [&] {
                        return sh.error != NTC_OK || next_task >= blocks.size() ||
                               (stop_batch >= 0 && (int64_t)batch_of(next_task) > stop_batch);
                    };
                    sh.cv.wait(g, [&] {
                        if (exhausted()) return true;
                        const uint64_t nb = batch_of(next_task);
                        const DSlot &sl = slot_of(nb);
                        return sl.batch == nb || sl.batch == ~0ULL;
                    });
                    if (exhausted()) return;
                    blk = next_task++;
                    b = batch_of(blk);
                    DSlot &sl = slot_of(b);
                    first = sl.batch != b;
                    if (first) {
                        DSlot fresh;
                        fresh.recs = sl.recs;
                        fresh.cap_recs = sl.cap_recs;
                        fresh.pay = sl.pay;
                        fresh.cap_pay = sl.cap_pay;
                        fresh.text = sl.text;
                        fresh.cap_text = sl.cap_text;
                        fresh.metas.swap(sl.metas);
                        sl = std::move(fresh);
                        sl.batch = b;
                        sl.first_block = batch_first(b);
                        sl.n_blocks = batch_end(b) - sl.first_block;
                        for (uint64_t i = 0; i < sl.n_blocks; i++) {
                            sl.n_recs += blocks[sl.first_block + i].n_recs;
                            sl.n_pay += blocks[sl.first_block + i].pay;
                        }
                        sl.metas.assign(sl.n_blocks, ntc_block_meta{});
                    }
                }
                DSlot &sl = slot_of(b);
                if (first) {  // size the batch's pinned record / stream buffer outside the lock
                    const bool okp = gpu_unpack ? ensure_pinned((void **)&sl.pay, &sl.cap_pay, sl.n_pay + 8)
                                                : ensure_pinned((void **)&sl.recs, &sl.cap_recs, sl.n_recs * 8 + 8);
                    if (!okp) {
                        sh.fail(NTC_ERR_HIP, "pinned host allocation failed");
                        return;
                    }
                    std::lock_guard<std::mutex> g(sh.mu);
                    sl.buffer = true;
                    sh.cv.notify_all();
                } else {
                    std::unique_lock<std::mutex> g(sh.mu);
                    sh.cv.wait(g, [&] { return sh.error != NTC_OK || sl.buffer; });
                    if (sh.error != NTC_OK) return;
                }
                uint64_t off = 0, poff = 0;
                for (uint64_t i = sl.first_block; i < blk; i++) {
                    off += blocks[i].n_recs;
                    poff += blocks[i].pay;
                }
                const auto tu = Clock::now();
                uint64_t used = 0, nr = 0, numr = 0, reads = 0, bases = 0;
                const DBlock &db = blocks[blk];
                int rc;
                if (db.bad) {
                    rc = NTC_ERR_FORMAT;
                    if (gpu_unpack) sl.metas[blk - sl.first_block].status = rc;
                } else if (gpu_unpack) {  // inflate only: the streams are decoded on the GPU
                    ntc_block_meta &m = sl.metas[blk - sl.first_block];
                    rc = ntc_read_block_streams(data + db.a, db.len, &used, sl.pay + poff, db.pay, &m);
                    if (rc == NTC_OK && (m.n_recs != db.n_recs || used != db.len)) rc = NTC_ERR_FORMAT;
                    for (int i = 0; i < 4; i++) m.stream[i].offset += poff;
                    if (rc != NTC_OK) m.status = rc;
                } else {
                    rc = ntc_read_block_into(data + db.a, db.len, &used, sl.recs + off, db.n_recs, &nr, &numr);
                    if (rc == NTC_OK && (nr != db.n_recs || used != db.len)) rc = NTC_ERR_FORMAT;
                    if (rc == NTC_OK) count_reads(sl.recs + off, nr, &reads, &bases);
                }
                add_time(t_unzip, secs(tu, Clock::now()));
                std::lock_guard<std::mutex> g(sh.mu);
                const int bi = (int)(blk - sl.first_block);
                if (rc != NTC_OK) {
                    if (sl.bad_block < 0 || bi < sl.bad_block) sl.bad_block = bi;
                    if (stop_batch < 0 || (int64_t)b < stop_batch) stop_batch = (int64_t)b;
                } else {
                    sl.n_reads += reads;  // recounted below when the batch holds a damaged block
                    sl.n_bases += bases;
                }
                sl.finished++;
                if (blk + 1 == blocks.size() || (stop_batch >= 0 && sl.finished == sl.n_blocks))
                    S.reader_done_s = secs(t0, Clock::now());
                if (sl.finished == sl.n_blocks) trace("inflated", b);
                if (!gpu_unpack && sl.finished == sl.n_blocks) assign_ahead();
                sh.cv.notify_all();
            }
        });

    // ---- assigner + writer (this thread) ------------------------------------------------------------
    struct stat ost;
    // pwrite only into a regular file opened without O_APPEND (Linux pwrite ignores the
    // offset under O_APPEND); the shared file offset is moved past the text at the end, so
    // `{ decode a; decode b; } > out` keeps both outputs as the reference's stdout does
    const int fl = fcntl(out_fd, F_GETFL);
    const bool seekable = fstat(out_fd, &ost) == 0 && S_ISREG(ost.st_mode) && fl >= 0 && !(fl & O_APPEND) &&
                          lseek(out_fd, 0, SEEK_CUR) >= 0;
    off_t out_pos = seekable ? lseek(out_fd, 0, SEEK_CUR) : 0;
    // one writer: buffered writes into one file serialise on its inode lock, and on the GPU
    // box one thread's pwrite put 1.6 GB into the page cache at 12.6 GB/s against 10.4 from
    // 8 threads at their own offsets and 1.9 through a shared mapping
    // (profiles/round5/write_bw_box.jsonl, scripts/write_bw.cpp)
    auto write_text = [&](const uint8_t *p, uint64_t n) -> bool {
        while (n) {
            const ssize_t w = seekable ? ::pwrite(out_fd, p, n, out_pos) : ::write(out_fd, p, n);
            if (w <= 0) return false;
            p += w;
            n -= (uint64_t)w;
            out_pos += w;
        }
        return true;
    };
    auto write_mate = [&](const uint8_t *p, uint64_t n) -> bool {
        while (n) {
            const ssize_t w = ::write(out_fd2, p, n);
            if (w < 0 && errno == EINTR) continue;
            if (w <= 0) return false;
            p += w;
            n -= (uint64_t)w;
        }
        return true;
    };
    for (uint64_t b = 0; b < n_batches; b++) {
        DSlot *slp;
        {
            std::unique_lock<std::mutex> g(sh.mu);
            sh.cv.wait(g, [&] {
                if (sh.error != NTC_OK) return true;
                if (stop_batch >= 0 && (int64_t)b > stop_batch) return true;
                assign_ahead();
                const DSlot &sl = slot_of(b);
                return sl.batch == b && sl.decoded;
            });
            if (sh.error != NTC_OK || (stop_batch >= 0 && (int64_t)b > stop_batch)) break;
            slp = &slot_of(b);
        }
        const auto tw = Clock::now();
        if (split) {  // the mate-1 records to out_fd, the mate-2 records to out_fd2
            const uint64_t f = std::min(slp->first_len, slp->text_len);
            if (!write_text(slp->text, f) || !write_mate(slp->text + f, slp->text_len - f)) sh.fail(NTC_ERR_IO, "write failed");
            PS.bytes1 += f;
            PS.bytes2 += slp->text_len - f;
            PS.pairs += slp->n_reads / 2;
        } else if (!discard && !write_text(slp->text, slp->text_len)) {
            sh.fail(NTC_ERR_IO, "write failed");
        }
        add_time(t_write, secs(tw, Clock::now()));
        std::lock_guard<std::mutex> g(sh.mu);
        if (b == 0) S.first_batch_s = secs(t0, Clock::now());
        trace("written", b);
        S.reads += slp->n_reads;
        S.bases += slp->n_bases;
        S.bytes_out += slp->text_len;
        S.blocks += slp->bad_block >= 0 ? (uint64_t)slp->bad_block : slp->n_blocks;
        const bool last = stop_batch >= 0 && (int64_t)b == stop_batch;
        slp->batch = ~0ULL;  // free the slot
        sh.cv.notify_all();
        if (last) break;
    }
    {
        std::lock_guard<std::mutex> g(sh.mu);
        if (sh.error == NTC_OK) sh.error = -1;  // stop the workers
        sh.cv.notify_all();
    }
    for (auto &t : pool) t.join();
    for (auto &t : gpus) t.join();
    for (auto &sl : slots) {
        pinned_free(sl.recs);
        pinned_free(sl.pay);
        pinned_free(sl.text);
    }
    if (data) munmap((void *)data, fsize);
    if (seekable) (void)lseek(out_fd, out_pos, SEEK_SET);
    int result = sh.error == -1 ? NTC_OK : sh.error;
    // every batch checked its own runs; one past the file's last read belongs to another encoding
    if (result == NTC_OK && stop_batch < 0 && nxf.n && nxf.runs[nxf.n - 1].read >= S.reads) {
        result = NTC_ERR_FORMAT;
        sh.msg = "exceptions: a run past the last read (the side file belongs to another encoding)";
    }
    // an input that ended cleanly used exactly all sections
    const bool clean_end = blocks.empty() ? fsize <= 32 : blocks.back().a + blocks.back().len == fsize;
    if (result == NTC_OK && stop_batch < 0 && clean_end && q_path && qf.n != blocks.size()) {
        result = NTC_ERR_FORMAT;
        sh.msg = "qualities: more sections than blocks (the side file belongs to another encoding)";
    }
    if (result == NTC_OK && stop_batch < 0 && clean_end && n_path && nf.n != blocks.size()) {
        result = NTC_ERR_FORMAT;
        sh.msg = "names: more sections than blocks (the side file belongs to another encoding)";
    }
    // under a digest file the lenient endings are errors: the file is known not to be whole
    if (result == NTC_OK && d_path && stop_batch >= 0) {
        result = NTC_ERR_FORMAT;
        char buf[120];
        std::snprintf(buf, sizeof(buf), "damaged block %llu: the output ends before it", (unsigned long long)S.blocks);
        sh.msg = buf;
    }
    if (result == NTC_OK && d_path && !clean_end) {
        result = NTC_ERR_FORMAT;
        sh.msg = "truncated input: the file ends inside a block";
    }
    if (result == NTC_OK && d_path && df.n != blocks.size()) {
        result = NTC_ERR_FORMAT;
        sh.msg = "digests: more sections than blocks (the input is truncated, or the side file belongs to another "
                 "encoding)";
    }
    S.dropped_blocks = blocks.size() - S.blocks;  // after a damaged block (or none)
    S.alloc_s += t_pin.load();
    S.parse_s = t_unzip.load();
    S.gpu_s = t_gpu.load();
    S.write_s = t_write.load();
    S.wall_s = secs(t0, Clock::now());
    S.threads = T;
    S.bad_read = result == NTC_ERR_DIGEST ? sh.bad_read : -1;
    if (ds) *ds = DS;
    if (pair_mode && discard) PS.pairs = S.reads / 2;
    if (ps) *ps = PS;
    if (result != NTC_OK)
        std::snprintf(S.error, sizeof(S.error), "%s", sh.msg.c_str());
    else if (stop_batch >= 0)  // not an error for the reference either: its loop just ends
        std::snprintf(S.error, sizeof(S.error), "damaged block %llu: output ends before it",
                      (unsigned long long)S.blocks);
    if (stats) *stats = S;
    return result;
}

int ntc_decode_file(ntc_ctx *const *ctxs, int n_ctx, const char *in_path, int out_fd, const ntc_pipeline_opts *opts,
                    ntc_pipeline_stats *stats) {
    return decode_file_impl(ctxs, n_ctx, in_path, nullptr, out_fd, opts, stats);
}

int ntc_decode_file_nx(ntc_ctx *const *ctxs, int n_ctx, const char *in_path, const char *nx_path, int out_fd,
                       const ntc_pipeline_opts *opts, ntc_pipeline_stats *stats) {
    return decode_file_impl(ctxs, n_ctx, in_path, nx_path, out_fd, opts, stats);
}

int ntc_decode_file_ex(ntc_ctx *const *ctxs, int n_ctx, const char *in_path, int out_fd, const ntc_file_opts *fo,
                       const ntc_pipeline_opts *opts, ntc_pipeline_stats *stats) {
    if (!fo) return NTC_ERR_INVALID_ARG;
    return decode_file_impl(ctxs, n_ctx, in_path, fo->nx_path, out_fd, opts, stats, fo->q_path);
}

int ntc_decode_file_ex2(ntc_ctx *const *ctxs, int n_ctx, const char *in_path, int out_fd, const ntc_file_opts2 *fo,
                        const ntc_pipeline_opts *opts, ntc_pipeline_stats *stats) {
    if (!fo || fo->struct_bytes < sizeof(ntc_file_opts2)) return NTC_ERR_INVALID_ARG;
    return decode_file_impl(ctxs, n_ctx, in_path, fo->nx_path, out_fd, opts, stats, fo->q_path, fo->n_path);
}

int ntc_decode_file_ex3(ntc_ctx *const *ctxs, int n_ctx, const char *in_path, int out_fd, const ntc_file_opts3 *fo,
                        const ntc_pipeline_opts *opts, ntc_pipeline_stats *stats, ntc_d_stats *d) {
    if (!fo || fo->struct_bytes < sizeof(ntc_file_opts3)) return NTC_ERR_INVALID_ARG;
    return decode_file_impl(ctxs, n_ctx, in_path, fo->nx_path, out_fd, opts, stats, fo->q_path, fo->n_path, fo->d_path, d,
                            true);
}

int ntc_decode_file_ex4(ntc_ctx *const *ctxs, int n_ctx, const char *in_path, int out_fd, const ntc_file_opts4 *fo,
                        const ntc_pipeline_opts *opts, ntc_pipeline_stats *stats, ntc_d_stats *d, ntc_p_stats *p) {
    if (!fo || fo->struct_bytes < sizeof(ntc_file_opts4)) return NTC_ERR_INVALID_ARG;
    return decode_file_impl(ctxs, n_ctx, in_path, fo->nx_path, out_fd, opts, stats, fo->q_path, fo->n_path, fo->d_path, d,
                            true, fo->pair_mode, fo->out_fd2, p);
}

}  // extern "C"
