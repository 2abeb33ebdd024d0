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
//
// The stages are member functions of Encoder (read_batches, run_gpu, deflate_worker,
// write_blocks), which holds what they share; ntc::pipe::encode_file checks the request, holds
// the contexts' modes for the call and runs them.  The decode pipeline follows below; what the
// two share (the request and stats bundles, the pinned pool, the threads' error state, the
// side streams' helpers) comes first.
#include <emmintrin.h>
#include <fcntl.h>
#include <hip/hip_runtime.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
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
#include "bgzf_core.h"
#include "digest_core.h"

namespace ntc {
namespace pipe {

// Everything the entry points (ntc_{en,de}code_file, _nx, _ex, _ex2, _ex3, _ex4,
// ntc_decode_file_ex5, ntc_encode_file_ex6 and ntc_decode_file_ex7) can say.  An entry point
// that lacks a field leaves it at its "none" value: mode 0, descriptor -1, path null.
struct FileJob {
    ntc_ctx *const *ctxs;
    int n_ctx;
    const char *in_path;
    int out_fd;
    const ntc_pipeline_opts *opts;
    // the side streams; encode reads the modes and descriptors, decode the paths
    ntc_file_opts4 fo{(uint32_t)sizeof(ntc_file_opts4), 0, -1, 0, -1, nullptr, nullptr, 0, -1, nullptr, 0, -1, nullptr, 0,
                      nullptr, -1};
    bool has_policy = false;   // false (ntc_encode_file): the contexts' policy as it is, no side file
    bool may_discard = false;  // decode _ex3 / _ex4: out_fd -1 runs everything but the text's copy and write
    uint64_t read_first = 0, read_count = 0;  // decode _ex5: the range of reads, count 0 = the whole file
    int inflate_engine = 0;                   // encode _ex6: NTC_INFLATE_*
    int out_format = 0;                       // decode _ex7: NTC_OUT_*
    FileJob(ntc_ctx *const *c, int n, const char *in, int out, const ntc_pipeline_opts *o)
        : ctxs(c), n_ctx(n), in_path(in), out_fd(out), opts(o) {}
    // the fields of ntc_file_opts, ntc_file_opts2 and ntc_file_opts3 (the same names in each)
    template <class FO>
    void take_ex(const FO &f) {
        has_policy = true;
        fo.nx_policy = f.nx_policy, fo.nx_fd = f.nx_fd, fo.nx_path = f.nx_path;
        fo.q_mode = f.q_mode, fo.q_fd = f.q_fd, fo.q_path = f.q_path;
    }
    template <class FO>
    void take_ex2(const FO &f) {
        take_ex(f);
        fo.n_mode = f.n_mode, fo.n_fd = f.n_fd, fo.n_path = f.n_path;
    }
    template <class FO>
    void take_ex3(const FO &f) {
        take_ex2(f);
        fo.d_mode = f.d_mode, fo.d_fd = f.d_fd, fo.d_path = f.d_path;
    }
};
// where the stats go; each may be null
struct FileStats {
    ntc_pipeline_stats *pipe = nullptr;
    ntc_nx_stats *nx = nullptr;
    ntc_q_stats *q = nullptr;
    ntc_n_stats *n = nullptr;
    ntc_d_stats *d = nullptr;
    ntc_p_stats *p = nullptr;
    ntc_r_stats *r = nullptr;
    ntc_i_stats *i = nullptr;
    ntc_z_stats *z = nullptr;
};
int encode_file(const FileJob &job, const FileStats &out);
int decode_file(const FileJob &job, const FileStats &out);

using Clock = std::chrono::steady_clock;
inline double secs(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double>(b - a).count(); }
inline void add_time(std::atomic<double> &a, double d) {
    double cur = a.load();
    while (!a.compare_exchange_weak(cur, cur + d)) {
    }
}

// Pinned host memory, pooled for the process
void *pinned_alloc(size_t n);
void pinned_free(void *q);

// the one mutex and condition variable of a pipeline's threads, and its first error
// (error -1: the writer is done, the workers stop)
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

// A context option held at `mode` on n contexts for the length of a call: set on all of them
// (rolled back if one refuses: rc() says so), back at 0 when the call leaves.  n = 0: nothing.
class ModeGuard {
  public:
    ModeGuard(int (*set)(ntc_ctx *, int), ntc_ctx *const *ctxs, int n, int mode) : set_(set), ctxs_(ctxs) {
        for (int i = 0; i < n && !rc_; i++)
            if ((rc_ = set_(ctxs_[i], mode))) n = i;
        n_ = mode ? n : 0;
        if (rc_) reset();
    }
    ~ModeGuard() { reset(); }
    ModeGuard(const ModeGuard &) = delete;
    ModeGuard &operator=(const ModeGuard &) = delete;
    int rc() const { return rc_; }

  private:
    void reset() {
        for (int i = 0; i < n_; i++) set_(ctxs_[i], 0);
        n_ = 0;
    }
    int (*set_)(ntc_ctx *, int);
    ntc_ctx *const *ctxs_;
    int n_ = 0, rc_ = NTC_OK;
};

// all of p[0, n) to fd
inline bool write_fd(int fd, const uint8_t *p, uint64_t n) {
    while (n) {
        const ssize_t w = ::write(fd, p, n);
        if (w < 0 && errno == EINTR) continue;
        if (w <= 0) return false;
        p += w;
        n -= (uint64_t)w;
    }
    return true;
}

}  // namespace pipe
}  // namespace ntc

namespace ntc {
NxHooks g_nx_hooks = {nullptr, nullptr, nullptr, nullptr};  // capi.cpp fills it at load
QHooks g_q_hooks = {nullptr, nullptr, nullptr, nullptr};
NHooks g_n_hooks = {nullptr, nullptr, nullptr};
DHooks g_d_hooks = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
PHooks g_p_hooks = {nullptr, nullptr, nullptr};
WHooks g_w_hooks = {nullptr};
ZHooks g_z_hooks = {nullptr, nullptr};
IHooks g_i_hooks = {nullptr, nullptr, nullptr};
BHooks g_b_hooks = {nullptr, nullptr};
}

namespace {
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
}  // namespace

void *ntc::pipe::pinned_alloc(size_t n) {
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
void ntc::pipe::pinned_free(void *q) {
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

namespace {
using namespace ntc::pipe;

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

constexpr uint64_t kPiece = 1u << 20;  // the gang scans and copies text in pieces of this size
// the newlines of p[0, len) and its first blank line, from the gang's scans of its pieces
void sum_scans(const std::vector<FqScan> &sc, const uint8_t *p, uint64_t *nl, uint64_t *blank) {
    *nl = 0, *blank = UINT64_MAX;
    for (uint64_t q = 0; q < sc.size(); q++) {
        const uint64_t a = q * kPiece;
        if (*blank == UINT64_MAX && a && p[a - 1] == '\n' && (p[a] == '\n' || p[a] == '\r')) *blank = a;
        if (*blank == UINT64_MAX && sc[q].blank != SIZE_MAX) *blank = a + sc[q].blank;
        *nl += sc[q].nl;
    }
}
// byte position just past newline `line` (1-based) of p[0, len): the piece holding it first
uint64_t cut_after_line(const std::vector<FqScan> &sc, const uint8_t *p, uint64_t len, uint64_t line) {
    uint64_t before = 0, q = 0;
    while (before + sc[q].nl < line) before += sc[q++].nl;
    const uint64_t a = q * kPiece;
    return a + nth_newline_end(p + a, std::min(len, a + kPiece) - a, line - before);
}

// a side section of a block (qualities, names): deflated with the streams, written to its file
template <class Meta>
struct SideSection {
    bool has = false;
    Meta meta{};
    uint8_t *sec = nullptr;
    uint64_t len = 0;
};
struct BlockOut {  // a deflated block (its four streams' parts), or a dropped one
    uint8_t *part[4] = {nullptr, nullptr, nullptr, nullptr};
    uint64_t len[4] = {0, 0, 0, 0};
    int status = NTC_OK;
    int left = 0;  // parts not yet deflated
    uint64_t n_reads = 0;            // the block's reads
    std::vector<ntc_nx_run> nx;      // its exception runs (policy keep), read relative to the block
    SideSection<ntc_qual_meta> q;    // quality mode keep / bin8
    SideSection<ntc_name_meta> n;    // names mode keep / id
    bool has_d = false;              // digests on: its section of the "NTCD" file
    ntc_digest_meta dmeta{};
    void free_parts() {
        for (int s = 0; s < 4; s++) ntc_buffer_free(part[s]);
        ntc_buffer_free(q.sec);
        ntc_buffer_free(n.sec);
    }
};

// deflate tasks: one per stream of a block (ntc_deflate_stream) and one per side section
enum class TaskKind { Stream, QualSection, NameSection };
struct Task {
    std::shared_ptr<uint8_t> payload;  // the GPU call's host payload (ntc_buffer_free)
    ntc_block_meta meta;
    uint64_t block;
    TaskKind kind;
    int stream;                        // Stream: 0..3
    std::shared_ptr<uint8_t> side;     // a section: the call's packed quality words / name sections
};

// what a context's encode call leaves beside the streams, fetched before its next call
struct SideData {
    std::vector<ntc_nx_run> runs;
    uint64_t nx_runs = 0, nx_bases = 0;
    std::vector<ntc_qual_meta> qmetas;
    std::vector<ntc_name_meta> nmetas;
    std::vector<ntc_digest_meta> dmetas;
    std::shared_ptr<uint8_t> qpl, npl, none;
};

struct TextSrc {  // one FASTQ input of the pair reader
    ntc_fastx *fx = nullptr;
    const uint8_t *map = nullptr;  // mapped plain text; null: streamed from a decoder
    uint64_t map_n = 0, pos = 0;   // mapped: the next record's start
    std::vector<uint8_t> pend;     // streamed: decoded text not yet sent
    bool at_end = false;           // streamed: the decoder has ended
    uint64_t sent = 0;             // text bytes sent so far
};

// The side streams that exist only where the GPU parses FASTQ text (DESIGN.md "Quality
// scores", "Read names", "Paired-end reads"): what the refusals say
struct TextOnly {
    const char *what, *lost, *not_fastq;
};
constexpr TextOnly kQualText = {"qualities", "quality lines", "FASTA has no quality lines"};
constexpr TextOnly kNameText = {"names", "header lines", "names are kept from FASTQ text only"};
constexpr TextOnly kPairText = {"pairs", "header lines", "mates are checked and woven in FASTQ text only"};

// One batch's side data of a context, one entry per block.  The hook is first called without
// buffers: it answers NTC_ERR_CAPACITY and the sizes; then again with room.  Anything but one
// entry per block is NTC_ERR_FORMAT (never expected).  call(metas, cap, payload, payload_cap,
// &n, &bytes) wraps the hook; a hook without a payload leaves bytes 0 and gets no buffer.
template <class Meta, class Call>
int collect_sections(uint64_t nblk, bool with_payload, std::vector<Meta> &metas, std::shared_ptr<uint8_t> &payload,
                     const Call &call) {
    uint64_t n = 0, bytes = 0;
    int r = call((Meta *)nullptr, 0, (uint8_t *)nullptr, 0, &n, &bytes);
    if (r == NTC_ERR_CAPACITY && n == nblk) {
        metas.resize(n);
        if (with_payload) payload.reset((uint8_t *)std::malloc(bytes ? bytes : 1), std::free);
        r = !with_payload || payload ? call(metas.data(), n, payload.get(), bytes, &n, &bytes) : NTC_ERR_CAPACITY;
    } else if (r == NTC_OK || r == NTC_ERR_CAPACITY) {
        r = NTC_ERR_FORMAT;
    }
    return r;
}

constexpr uint32_t BR = 65536;  // main.rs:152

struct Encoder {
    // ---- the request (fixed before the threads start) -----------------------------------------
    ntc_ctx *const *ctxs;
    const int n_ctx, out_fd;
    const ntc_file_opts4 &fo;  // the side streams' modes and descriptors
    const int policy;          // -1: the contexts as they are
    const bool keep;
    int engine = 0, q_coder = 0, RT = 1;  // RT: the reader's gang
    bool gpu_deflate = false;  // NTC_DEFLATE_GPU: the calls return members; engine then serves the side sections
    uint64_t per_batch = 0, d_nodes = 0;
    uint32_t nx_sub = 0, d_k = 0;
    ntc_fastx *fx = nullptr, *fx2 = nullptr;
    const uint8_t *text = nullptr;  // a mapped plain FASTQ goes to the GPU as text
    uint64_t text_n = 0;
    bool streamed = false;
    Clock::time_point t0;
    uint64_t etrace_n = 0;
    // ---- shared by the threads, under sh.mu ----------------------------------------------------
    Shared sh;
    int NB = 0;
    std::vector<Batch> ring;
    std::vector<std::deque<int>> gpu_q;  // per context: ring indices in batch order
    bool reader_done = false;
    uint64_t total_blocks = 0;  // known once the reader is done
    std::deque<Task> tasks;
    std::map<uint64_t, BlockOut> done;  // blocks in progress
    uint64_t pending_tasks = 0;
    uint64_t writer_at = 0;    // the block the writer waits for
    uint64_t max_pending = 0;  // bound on blocks queued or finished but unwritten
    ntc_pipeline_stats S{};
    ntc_nx_stats NX{};
    ntc_q_stats QS{};  // ... and the writer's
    ntc_n_stats NS{};
    ntc_d_stats DS{};
    std::atomic<double> t_pin{0}, t_parse{0}, t_gpu{0}, t_deflate{0}, t_write{0};
    // ---- the reader's -----------------------------------------------------------------------------
    // GPU-parse reader state.  Mapped: the next batch's text starts at text_pos (a record
    // start).  Streamed (a decoder's output): the text after the last cut, carry_n bytes at
    // carry_p in the previous batch's buffer, goes first into the next one.
    TextSrc msrc[2];
    uint64_t text_pos = 0;
    const uint8_t *carry_p = nullptr;
    uint64_t carry_n = 0;
    bool stream_eof = false;
    double rec_bytes = 320;  // text bytes per record so far (a guess for 150 bp reads until known)
    std::atomic<uint64_t> text_batches{0};
    uint64_t next_read = 0, next_block = 0, batch_no = 0;
    int prev = -1;
    uint64_t carry = 0;  // reads at the tail of ring[prev] past its processed blocks

    Encoder(const FileJob &job, int policy_)
        : ctxs(job.ctxs), n_ctx(job.n_ctx), out_fd(job.out_fd), fo(job.fo), policy(policy_), keep(policy_ == NTC_NX_KEEP) {}

    // NTC_PIPE_TRACE=n: the first n batches' (and blocks') events on stderr, ms from the start
    void etrace(const char *what, uint64_t b) const {
        if (b < etrace_n) std::fprintf(stderr, "[pipe] %8.3f ms %s %llu\n", 1e3 * secs(t0, Clock::now()), what,
                                       (unsigned long long)b);
    }
    bool pin_text(Batch &b, uint64_t cap, bool keep_carry);
    int fill_text(ntc::Gang &gang, Batch &b, bool &eof);
    int fill_pair(ntc::Gang &gang, Batch &b, bool &eof);
    int fill_host(Batch &b, int bi);
    void hand_over(Batch &b, int bi);
    void read_batches();
    bool collect_side(int c, uint64_t nblk, SideData &sd);
    void run_gpu(int c);
    void deflate_worker();
    void write_side(BlockOut &out, uint64_t reads_written);
    void write_blocks();
};

// (re)pin b's text buffer at cap bytes; keep_carry: the carried text it holds moves along
bool Encoder::pin_text(Batch &b, uint64_t cap, bool keep_carry) {
    const auto ta = Clock::now();
    uint8_t *nt = (uint8_t *)pinned_alloc(cap);
    if (!nt) return false;
    if (keep_carry && carry_n && carry_p == b.text) {  // growing the buffer that holds the carry
        std::memcpy(nt, carry_p, carry_n);
        carry_p = nt;
    }
    pinned_free(b.text);
    b.text = nt;
    b.text_cap = cap;
    t_pin = t_pin.load() + secs(ta, Clock::now());  // the reader alone writes it
    return true;
}

// Fill b with the text of the next whole blocks (or the input's end): 1 = filled, 0 = no
// input left, -1 = hand over to the host parser (a blank line before the cut, a line
// count that is not a multiple of 4 at the end, a block too large for one call), -2 = the
// decoder failed
int Encoder::fill_text(ntc::Gang &gang, Batch &b, bool &eof) {
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
        if (b.text_cap < want_cap && !pin_text(b, want_cap, true)) return -1;
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
        uint64_t nl, blank;  // the first blank line in the text read
        sum_scans(sc, src, &nl, &blank);
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
            cut = cut_after_line(sc, src, len, 4 * n);  // the batch ends after newline 4 n
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
}

// The same for two mate inputs (mate_path): the next n records of each, the same n from
// both -- 2 n a multiple of 65,536, or the inputs' end -- into b's one pinned buffer at two
// offsets, for the GPU to weave.  The host newline counts make the cuts exact.  1 = filled,
// 0 = no input left, -1 = a text the GPU cannot take (as above), -2 = a decoder failed, -3 =
// one input ended while the other still holds a record
int Encoder::fill_pair(ntc::Gang &gang, Batch &b, bool &eof) {
    const uint64_t kMaxHalf = ((1ull << 32) - (64u << 20)) / 2;  // both texts in one call of < 4 GiB
    const uint64_t half = per_batch / 2;
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
            uint64_t nl;
            sum_scans(x.sc, x.p, &nl, &x.blank);
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
        if (!last && !(x.end && x.recs == n)) x.cut = cut_after_line(x.sc, x.p, x.len, 4 * n);  // the batch ends after newline 4 n
        if (x.blank < x.cut) return -1;  // a blank line: only the host parser takes it
    }
    const uint64_t at2 = (w[0].cut + 63) & ~63ull, need = at2 + w[1].cut + 64;
    if (b.text_cap < need && !pin_text(b, need + need / 8, false)) return -1;
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
}

// The host parser's batch into b (ring slot bi): the previous buffer's carry, then reads until
// the buffer holds at least one whole block (or the input ends).  A buffer that cannot hold a
// whole 65,536-read block (long reads) grows until it does.  1 = go on, 0 = the input's end,
// -1 = failed (sh says why)
int Encoder::fill_host(Batch &b, int bi) {
    auto grow = [](Batch &b, uint64_t need_bases, uint64_t keep_bases) -> bool {
        if (need_bases <= b.cap_bases) return true;
        const uint64_t cap = std::max(need_bases, b.cap_bases * 2);
        uint8_t *nbuf = (uint8_t *)pinned_alloc(cap);
        if (!nbuf) return false;
        if (keep_bases) std::memcpy(nbuf, b.bases, keep_bases);
        pinned_free(b.bases);
        b.bases = nbuf;
        b.cap_bases = cap;
        return true;
    };
    if (!b.bases) {
        const auto ta = Clock::now();
        if (!(b.bases = (uint8_t *)pinned_alloc(b.cap_bases))) {
            sh.fail(NTC_ERR_HIP, "pinned host allocation failed");
            return -1;
        }
        t_pin = t_pin.load() + secs(ta, Clock::now());  // the reader alone writes it
    }
    uint64_t used = 0;  // bases in b
    b.offs[0] = 0;
    if (carry) {  // the previous buffer's unprocessed reads go first
        const Batch &p = ring[(size_t)prev];
        const uint64_t a0 = p.offs[p.n_process], a1 = p.offs[p.n_reads];
        if (!grow(b, (a1 - a0) * 2 + (64u << 20), 0)) {
            sh.fail(NTC_ERR_CAPACITY, "pinned host allocation failed");
            return -1;
        }
        std::memcpy(b.bases, p.bases + a0, a1 - a0);
        for (uint64_t r = 0; r <= carry; r++) b.offs[r] = p.offs[p.n_process + r] - a0;
        used = a1 - a0;
    }
    b.n_reads = carry;
    bool eof = false;
    const auto tp = Clock::now();
    for (;;) {  // fill: at least one whole block (or the end of the input)
        const uint64_t room = b.cap_bases - used;
        const uint64_t want = per_batch - b.n_reads, max_b = room / 2;
        uint64_t got = 0;
        const int r = ntc_fastx_next_batch_into(fx, want, max_b, b.bases + used, room, b.offs + b.n_reads, &got);
        if (r) {
            sh.fail(r, r == NTC_ERR_CAPACITY ? "a read longer than half the batch buffer (raise batch_bases)"
                                             : "FASTX input: malformed or unreadable");
            add_time(t_parse, secs(tp, Clock::now()));
            return -1;
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
        if (!grow(b, b.cap_bases * 2, used)) {
            sh.fail(NTC_ERR_CAPACITY, "pinned host allocation failed");
            add_time(t_parse, secs(tp, Clock::now()));
            return -1;
        }
    }
    add_time(t_parse, secs(tp, Clock::now()));
    if (batch_no == 0) S.first_batch_s = secs(t0, Clock::now());
    b.n_process = eof ? b.n_reads : (b.n_reads / BR) * BR;
    carry = b.n_reads - b.n_process;
    prev = bi;
    if (b.n_process) hand_over(b, bi);
    return eof && carry == 0 ? 0 : 1;
}

// b (ring slot bi) is the next batch: numbered, and queued for its context's driver
void Encoder::hand_over(Batch &b, int bi) {
    b.first_read = next_read;
    b.first_block = next_block;
    next_read += b.n_process;
    next_block += (b.n_process + BR - 1) / BR;
    if (b.is_text) {
        text_batches++;
        etrace("read batch", batch_no);
    }
    std::lock_guard<std::mutex> g(sh.mu);
    b.busy = true;
    gpu_q[(size_t)(batch_no % (uint64_t)n_ctx)].push_back(bi);
    batch_no++;
    sh.cv.notify_all();
}

// ---- reader -----------------------------------------------------------------------------------
void Encoder::read_batches() {
    const char *mate_path = fo.mate_path;
    bool as_text = text != nullptr || streamed || mate_path;  // (a mate input that is no text failed before)
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
                hand_over(b, bi);
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
            if (fo.pair_mode || fo.q_mode || fo.n_mode) {
                const TextOnly &t = fo.pair_mode ? kPairText : fo.q_mode ? kQualText : kNameText;
                sh.fail(NTC_ERR_UNSUPPORTED, std::string(t.what) + ": a blank line, or records that are not four lines each: "
                                             "this batch needs the host parser, which drops the " + t.lost, (int64_t)next_read);
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
        if (fill_host(b, bi) <= 0) break;
    }
    std::lock_guard<std::mutex> g(sh.mu);
    S.reader_done_s = secs(t0, Clock::now());
    reader_done = true;
    total_blocks = next_block;
    S.reads = next_read;
    sh.cv.notify_all();
}

// ---- GPU drivers --------------------------------------------------------------------------
// After context c's encode call of nblk blocks, before its next one: the batch's exception
// runs (policy keep) and counts, its quality sections (mode keep / bin8) and name sections
// (mode keep / id), one per block, and its digests (digests on), one entry per block.
// false: failed (sh says why)
bool Encoder::collect_side(int c, uint64_t nblk, SideData &sd) {
    ntc_ctx *ctx = ctxs[c];
    if (policy > 0) {
        const ntc::NxHooks &hk = ntc::g_nx_hooks;
        hk.last_counts(ctx, nullptr, &sd.nx_runs, &sd.nx_bases);
        uint64_t nrun = 0;
        int rx = NTC_OK;
        if (keep && hk.encode_exceptions(ctx, nullptr, 0, &nrun) == NTC_ERR_CAPACITY) {
            sd.runs.resize(nrun);
            rx = hk.encode_exceptions(ctx, sd.runs.data(), nrun, &nrun);
        }
        if (rx) {
            sh.fail(rx, std::string("encode: ") + ntc_last_error(ctx));
            return false;
        }
    }
    const char *what = "qualities";
    int r = NTC_OK;
    if (fo.q_mode)
        r = collect_sections(nblk, true, sd.qmetas, sd.qpl, [&](auto *m, uint64_t cap, uint8_t *p, uint64_t pcap, uint64_t *n,
                                                                uint64_t *bytes) {
            return ntc::g_q_hooks.encode_qualities(ctx, m, cap, p, pcap, n, bytes);
        });
    if (!r && fo.n_mode) {
        what = "names";
        r = collect_sections(nblk, true, sd.nmetas, sd.npl, [&](auto *m, uint64_t cap, uint8_t *p, uint64_t pcap, uint64_t *n,
                                                                uint64_t *bytes) {
            return ntc::g_n_hooks.encode_names(ctx, m, cap, p, pcap, n, bytes);
        });
    }
    if (!r && fo.d_mode) {
        what = "digests";
        r = collect_sections(nblk, false, sd.dmetas, sd.none,
                             [&](auto *m, uint64_t cap, uint8_t *, uint64_t, uint64_t *n, uint64_t *) {
                                 return ntc::g_d_hooks.encode_digests(ctx, m, cap, n);
                             });
    }
    if (r) sh.fail(r, std::string("encode: ") + what + ": " + ntc_last_error(ctx));
    return !r;
}

void Encoder::run_gpu(int c) {
    const ntc::PHooks &ph = ntc::g_p_hooks;
    const int q_mode = fo.q_mode, n_mode = fo.n_mode, d_mode = fo.d_mode, pair_mode = fo.pair_mode;
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
        SideData sd;
        if (!collect_side(c, nblk, sd)) return;
        // NTC_DEFLATE_GPU: the payload holds the streams' members; a block's parts are copies of
        // them behind their headers, and nothing of it goes to the pool but its side sections
        std::vector<uint64_t> members;
        std::vector<uint8_t *> parts;
        if (gpu_deflate) {
            uint64_t got = 0;
            members.resize(nblk * 8);
            const int rm = ntc::g_z_hooks.encode_members(ctxs[c], members.data(), nblk, &got);
            if (rm || got != nblk) {
                sh.fail(rm ? rm : NTC_ERR_FORMAT, std::string("encode: members: ") + ntc_last_error(ctxs[c]));
                return;
            }
            parts.assign(nblk * 4, nullptr);
            const auto drop_parts = [&] {
                for (uint8_t *p : parts) ntc_buffer_free(p);
            };
            for (uint64_t k = 0; k < nblk; k++) {
                if (metas[k].status == NTC_ERR_EMPTY_READ) continue;
                if (metas[k].status != NTC_OK) {
                    drop_parts();
                    sh.fail(metas[k].status, "malformed block");
                    return;
                }
                for (int s = 0; s < 4; s++) {
                    const uint64_t off = members[k * 8 + 2 * s], len = members[k * 8 + 2 * s + 1];
                    uint8_t *p = off + len <= plen && len >= 18 ? (uint8_t *)std::malloc(32 + len) : nullptr;
                    if (!p) {
                        drop_parts();
                        sh.fail(NTC_ERR_CAPACITY, "encode: members: allocation");
                        return;
                    }
                    ntc::stream_header(p, metas[k], s, len);
                    std::memcpy(p + 32, payload + off, len);
                    parts[k * 4 + s] = p;
                }
            }
            pl.reset();
        }
        const std::vector<ntc_nx_run> &runs = sd.runs;
        etrace("gpu done, first block", b.first_block);
        std::lock_guard<std::mutex> g(sh.mu);
        S.gpu_done_s = secs(t0, Clock::now());
        S.bases += b.is_text ? nb : b.offs[b.n_process] - b.offs[0];
        NX.bases += sd.nx_bases;
        if (policy == NTC_NX_MASK) NX.runs += sd.nx_runs;
        b.busy = false;
        size_t run_at = 0;
        for (uint64_t k = 0; k < nblk; k++) {  // streams of the largest payload first
            const bool ok = metas[k].status == NTC_OK;
            const uint64_t blk = b.first_block + k;
            BlockOut &bo = done[blk];
            bo.status = metas[k].status;
            bo.n_reads = metas[k].num_records;
            for (; run_at < runs.size() && runs[run_at].read < (k + 1) * (uint64_t)BR; run_at++) {
                bo.nx.push_back(runs[run_at]);
                bo.nx.back().read -= k * (uint64_t)BR;
            }
            bo.left = gpu_deflate ? 0 : ok ? 4 : 1;
            for (int q = 0; q < 4 && gpu_deflate && ok; q++) {
                bo.part[q] = parts[k * 4 + q];
                bo.len[q] = 32 + members[k * 8 + 2 * q + 1];
            }
            if (q_mode && ok) {  // a dropped block takes its section with it
                bo.q.has = true;
                bo.q.meta = sd.qmetas[k];
                bo.left++;
                tasks.push_back(Task{pl, metas[k], blk, TaskKind::QualSection, 0, sd.qpl});
            }
            if (n_mode && ok) {
                bo.n.has = true;
                bo.n.meta = sd.nmetas[k];
                bo.left++;
                tasks.push_back(Task{pl, metas[k], blk, TaskKind::NameSection, 0, sd.npl});
            }
            if (d_mode && ok) {  // (nothing to deflate: the writer puts the 56 bytes out)
                bo.has_d = true;
                bo.dmeta = sd.dmetas[k];
            }
            int order[4] = {0, 1, 2, 3};
            std::sort(order, order + 4, [&](int x, int y) {
                return metas[k].stream[x].encoded_size > metas[k].stream[y].encoded_size;
            });
            for (int q = 0; q < (ok ? 4 : 1) && !gpu_deflate; q++)
                tasks.push_back(Task{pl, metas[k], blk, TaskKind::Stream, order[q], nullptr});
            pending_tasks++;
        }
        sh.cv.notify_all();
    }
}

// ---- deflate pool ----------------------------------------------------------------------------
void Encoder::deflate_worker() {
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
        if (status == NTC_OK && task.kind != TaskKind::Stream) {  // a side section: its meta is the block's
            const bool is_q = task.kind == TaskKind::QualSection;
            ntc_qual_meta qm{};
            ntc_name_meta nm{};
            {
                std::lock_guard<std::mutex> g(sh.mu);
                if (is_q) qm = done[task.block].q.meta;
                else nm = done[task.block].n.meta;
            }
            const int r = is_q ? ntc_q_deflate_section(&qm, task.side.get() + qm.payload_off, engine, &data, &len)
                               : ntc_n_deflate_section(&nm, task.side.get() + nm.payload_off, engine, &data, &len);
            if (r) {
                sh.fail(r, is_q ? "qualities: deflate failed" : "names: deflate failed");
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
        task.side.reset();
        add_time(t_deflate, secs(td, Clock::now()));
        std::lock_guard<std::mutex> g(sh.mu);
        BlockOut &bo = done[task.block];
        if (task.kind == TaskKind::QualSection) {
            bo.q.sec = data;
            bo.q.len = len;
        } else if (task.kind == TaskKind::NameSection) {
            bo.n.sec = data;
            bo.n.len = len;
        } else {
            bo.part[task.stream] = data;
            bo.len[task.stream] = len;
        }
        if (--bo.left == 0) sh.cv.notify_all();
    }
}

// ---- writer (the calling thread) -------------------------------------------------------------
// A written block's part of every side file: its exception runs, `read` counted over the reads
// of the blocks written so far (what decode will print as seq.N - 1), and its sections
void Encoder::write_side(BlockOut &out, uint64_t reads_written) {
    if (!out.nx.empty()) {
        uint64_t last_read = UINT64_MAX;
        for (auto &r : out.nx) {
            NX.reads += r.read != last_read;
            last_read = r.read;
            r.read += reads_written;
        }
        if (ntc_nx_write(fo.nx_fd, out.nx.data(), out.nx.size(), nx_sub, 0)) sh.fail(NTC_ERR_IO, "exceptions: write failed");
        NX.runs += out.nx.size();
    }
    if (out.q.has) {
        if (!write_fd(fo.q_fd, out.q.sec, out.q.len)) sh.fail(NTC_ERR_IO, "qualities: write failed");
        QS.sections++;
        QS.quals += out.q.meta.n_quals;
        QS.packed_bytes += out.q.meta.payload_bytes;
        // coder 1 (no gzip member): the section as written
        QS.deflated_bytes += out.q.meta.reserved[0] == 1 ? out.q.len : out.q.len - 24 - out.q.meta.n_syms;
    }
    if (out.n.has) {
        if (!write_fd(fo.n_fd, out.n.sec, out.n.len)) sh.fail(NTC_ERR_IO, "names: write failed");
        NS.sections++;
        NS.names += out.n.meta.n_reads;
        NS.name_bytes += out.n.meta.name_bytes;
        NS.payload_bytes += out.n.meta.payload_bytes;
        NS.deflated_bytes += out.n.len - 32;
    }
    if (out.has_d) {
        if (const int rd = ntc_d_write_section(fo.d_fd, &out.dmeta))
            sh.fail(rd == NTC_ERR_IO ? rd : NTC_ERR_FORMAT, "digests: write failed");
        DS.sections++;
        DS.blocks_seq += out.dmeta.components & ntc::kDgSeq ? 1 : 0;
        DS.blocks_sym += out.dmeta.components & ntc::kDgSym ? 1 : 0;
        DS.blocks_qual += out.dmeta.components & ntc::kDgQual ? 1 : 0;
        DS.blocks_name += out.dmeta.components & ntc::kDgName ? 1 : 0;
    }
}

void Encoder::write_blocks() {
    uint8_t header[32];
    ntc_file_header(header);
    if (!write_fd(out_fd, header, 32)) sh.fail(NTC_ERR_IO, "write failed");
    S.bytes_out = 32;
    // the side files: their headers now, then a section per written block (the exceptions: per
    // written block that has runs), in file order
    if (keep && ntc_nx_write(fo.nx_fd, nullptr, 0, nx_sub, 1)) sh.fail(NTC_ERR_IO, "exceptions: write failed");
    if (fo.q_mode && ntc_q_write_header2(fo.q_fd, fo.q_mode, q_coder)) sh.fail(NTC_ERR_IO, "qualities: write failed");
    if (fo.n_mode && ntc_n_write_header(fo.n_fd, fo.n_mode)) sh.fail(NTC_ERR_IO, "names: write failed");
    // the components the digest file can hold: what the modes of this call yield
    const uint32_t d_components = ntc::kDgSeq | (keep ? ntc::kDgSym : 0) | (fo.q_mode ? ntc::kDgQual : 0) |
                                  (fo.n_mode ? ntc::kDgName : 0);
    if (fo.d_mode && ntc_d_write_header(fo.d_fd, d_components, d_k, d_nodes)) sh.fail(NTC_ERR_IO, "digests: write failed");
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
                if (!write_fd(out_fd, out.part[q], out.len[q])) sh.fail(NTC_ERR_IO, "write failed");
                S.bytes_out += out.len[q];
            }
            S.blocks++;
            write_side(out, reads_written);
            reads_written += out.n_reads;
        } else {
            S.dropped_blocks++;
            NX.runs_in_dropped_blocks += out.nx.size();
        }
        out.free_parts();
        add_time(t_write, secs(tw, Clock::now()));
        etrace("written block", blk);
    }
    std::lock_guard<std::mutex> g(sh.mu);
    if (sh.error == NTC_OK) sh.error = -1;  // stop the workers (no more tasks will come)
    sh.cv.notify_all();
}

// mode in [0, max_mode] with its descriptor (mode 0: -1), and the GPU stage there for it
int check_side(int mode, int max_mode, int fd, bool supported) {
    if (mode < 0 || mode > max_mode || (mode ? fd < 0 : fd != -1)) return NTC_ERR_INVALID_ARG;
    return mode && !supported ? NTC_ERR_UNSUPPORTED : NTC_OK;
}

}  // namespace

int ntc::pipe::encode_file(const FileJob &job, const FileStats &stats) {
    ntc_ctx *const *ctxs = job.ctxs;
    const int n_ctx = job.n_ctx;
    const ntc_file_opts4 &fo = job.fo;
    if (!ctxs || n_ctx <= 0 || !job.in_path || job.out_fd < 0) return NTC_ERR_INVALID_ARG;
    for (int i = 0; i < n_ctx; i++)
        if (!ctxs[i]) return NTC_ERR_INVALID_ARG;
    // the side streams' arguments, in the order the entry points grew: pairs, qualities, names,
    // digests, then the policy (the tests pin which error wins)
    const int pair_mode = fo.pair_mode, q_mode = fo.q_mode, n_mode = fo.n_mode, d_mode = fo.d_mode;
    if (pair_mode < 0 || pair_mode > 2 || (!pair_mode && fo.mate_path)) return NTC_ERR_INVALID_ARG;
    const ntc::PHooks &ph = ntc::g_p_hooks;
    if (pair_mode && (!ph.set_mode || !ph.encode_paired)) return NTC_ERR_UNSUPPORTED;
    const ntc::QHooks &qh = ntc::g_q_hooks;
    if (const int r = check_side(q_mode, 2, fo.q_fd, qh.set_mode && qh.encode_qualities)) return r;
    // the sections' coder is the contexts' "quality_coder" option, which must be the same in all
    int q_coder = 0;
    if (q_mode && qh.get_coder) {
        q_coder = qh.get_coder(ctxs[0]);
        for (int i = 0; i < n_ctx; i++)
            if (q_coder < 0 || qh.get_coder(ctxs[i]) != q_coder) return NTC_ERR_INVALID_ARG;
    }
    const ntc::NHooks &nh = ntc::g_n_hooks;
    if (const int r = check_side(n_mode, 2, fo.n_fd, nh.set_mode && nh.encode_names)) return r;
    const ntc::DHooks &dh = ntc::g_d_hooks;
    if (const int r = check_side(d_mode, 1, fo.d_fd, dh.set_mode && dh.encode_digests && dh.index_info)) return r;
    const int policy = job.has_policy ? fo.nx_policy : -1;
    const ntc::NxHooks &hk = ntc::g_nx_hooks;
    if (policy >= 0) {
        if (policy > NTC_NX_KEEP || (policy == NTC_NX_KEEP ? fo.nx_fd < 0 : fo.nx_fd != -1)) return NTC_ERR_INVALID_ARG;
        if (policy != NTC_NX_ERROR && (!hk.set_policy || !hk.last_counts || !hk.encode_exceptions))
            return NTC_ERR_UNSUPPORTED;
    }
    // the contexts leave the call under policy error, with qualities and names dropped, digests
    // and pairs off
    ModeGuard policy_guard(hk.set_policy, ctxs, policy >= 0 && hk.set_policy ? n_ctx : 0, policy);
    if (policy_guard.rc()) return policy_guard.rc();
    Encoder E(job, policy);
    if (policy > 0) {
        hk.last_counts(ctxs[0], &E.nx_sub, nullptr, nullptr);
        if (!E.nx_sub) return NTC_ERR_NO_INDEX;
    }
    ModeGuard q_guard(qh.set_mode, ctxs, q_mode ? n_ctx : 0, q_mode);
    if (q_guard.rc()) return q_guard.rc();
    ModeGuard n_guard(nh.set_mode, ctxs, n_mode ? n_ctx : 0, n_mode);
    if (n_guard.rc()) return n_guard.rc();
    if (d_mode)
        if (int r = dh.index_info(ctxs[0], &E.d_nodes, &E.d_k)) return r;
    ModeGuard d_guard(dh.set_mode, ctxs, d_mode ? n_ctx : 0, 1);
    if (d_guard.rc()) return d_guard.rc();
    ModeGuard p_guard(ph.set_mode, ctxs, pair_mode ? n_ctx : 0, pair_mode);
    if (p_guard.rc()) return p_guard.rc();

    ntc_pipeline_opts o{};
    if (job.opts) o = *job.opts;
    // NTC_INFLATE_GPU: the reader's BGZF runs go through an inflater on the first context's device
    const ntc::IHooks &ih = ntc::g_i_hooks;
    if (job.inflate_engine != NTC_INFLATE_HOST && job.inflate_engine != NTC_INFLATE_GPU) return NTC_ERR_INVALID_ARG;
    const bool gpu_inflate = job.inflate_engine == NTC_INFLATE_GPU;
    if (gpu_inflate && o.host_parse) return NTC_ERR_INVALID_ARG;
    if (gpu_inflate && (!ih.create || !ih.run || !ih.destroy)) return NTC_ERR_UNSUPPORTED;
    // NTC_DEFLATE_GPU: the contexts deflate behind their packer ("gpu_deflate"); the side sections stay
    // with the pool, under the engine `--deflate auto` stands for
    const ntc::ZHooks &zh = ntc::g_z_hooks;
    E.gpu_deflate = o.deflate_engine == NTC_DEFLATE_GPU;
    if (E.gpu_deflate && (!zh.set_mode || !zh.encode_members)) return NTC_ERR_UNSUPPORTED;
    ModeGuard z_guard(zh.set_mode, ctxs, E.gpu_deflate ? n_ctx : 0, 1);
    if (z_guard.rc()) return z_guard.rc();
    if (E.gpu_deflate) o.deflate_engine = ntc::libdeflate_loaded() ? NTC_DEFLATE_ADAPTIVE : NTC_DEFLATE_ZLIB;
    const int T = o.threads > 0 ? o.threads : ntc_host_threads();
    // 4 blocks per GPU call and 64 Mi-base buffers: the first batch is on the GPU after
    // ~30 ms and the pinned ring stays small (10 M x 150 bp: pipeline 0.59 -> 0.32 s against
    // 16 blocks and 256 Mi bases, scripts/pipe_bench.py on one MI355X box)
    E.per_batch = (uint64_t)(o.blocks_per_batch > 0 ? o.blocks_per_batch : 4) * BR;
    const uint64_t cap_bases = o.batch_bases > 0 ? o.batch_bases : (64ull << 20);
    E.engine = o.deflate_engine;
    E.q_coder = q_coder;
    E.max_pending = (uint64_t)T * 8 + 64;
    ntc_pipeline_stats &S = E.S;
    const auto t0 = E.t0 = Clock::now();
    const char *etr = std::getenv("NTC_PIPE_TRACE");
    E.etrace_n = etr ? (uint64_t)std::atoll(etr) : 0;

    ntc_fastx *&fx = E.fx, *&fx2 = E.fx2;
    // `--inflate gpu`: one inflater, made before the inputs are opened so that their readers use it
    // from the first member on
    ntc::Inflater *inflater = nullptr;
    if (gpu_inflate)
        if (const int irc = ih.create(ctxs[0], &inflater)) return irc;
    const auto open_input = [&](const char *path, ntc_fastx **out) {
        return inflater ? ntc::fastx_open_inflating(path, inflater, out) : ntc_fastx_open(path, out);
    };
    int rc = open_input(job.in_path, &fx);
    if (rc) {
        if (inflater) ih.destroy(inflater);
        return rc;
    }
    ntc_fastx_set_threads(fx, T);
    E.text = o.host_parse ? nullptr : ntc::fastx_mapped(fx, &E.text_n);
    // the mate-2 input goes through the same ingest; the two decoders share the thread budget
    if (fo.mate_path) {
        if ((rc = open_input(fo.mate_path, &fx2))) {
            ntc_fastx_close(fx);
            if (inflater) ih.destroy(inflater);
            return rc;
        }
        ntc_fastx_set_threads(fx, std::max(1, T / 2));
        ntc_fastx_set_threads(fx2, std::max(1, T / 2));
    }
    // ... and every input must be BGZF, read member by member
    if (gpu_inflate) {
        const char *not_bgzf = !ntc::fastx_is_bgzf(fx) ? job.in_path : fx2 && !ntc::fastx_is_bgzf(fx2) ? fo.mate_path : nullptr;
        if (not_bgzf) {
            ntc_fastx_close(fx);
            if (fx2) ntc_fastx_close(fx2);
            ih.destroy(inflater);
            if (stats.pipe) {
                *stats.pipe = ntc_pipeline_stats{};
                stats.pipe->bad_read = -1;
                std::snprintf(stats.pipe->error, sizeof(stats.pipe->error), "inflate gpu: %s does not start with a BGZF member",
                              not_bgzf);
            }
            return NTC_ERR_UNSUPPORTED;
        }
    }

    // pinned ring: the GPU threads hold at most n_ctx buffers, the reader fills one more.
    // A slot's base buffer (the large part, ~320 MB) is pinned by the reader when it first
    // fills the slot, so only the first one delays the first batch (pinning runs at a few
    // GB/s); the offsets are pinned here.
    E.NB = n_ctx + 2;
    std::vector<Batch> &ring = E.ring;
    ring.resize((size_t)E.NB);
    for (auto &b : ring) {
        b.cap_bases = cap_bases + BR * 1024ull;  // a carry of < 65,536 reads sits in front
        b.cap_reads = E.per_batch + BR + 1;
        if (!(b.offs = (uint64_t *)pinned_alloc(b.cap_reads * 8))) {
            for (auto &x : ring) pinned_free(x.offs);
            ntc_fastx_close(fx);
            if (fx2) ntc_fastx_close(fx2);
            if (inflater) ih.destroy(inflater);
            return NTC_ERR_HIP;
        }
    }
    S.alloc_s = secs(t0, Clock::now());
    E.gpu_q.resize((size_t)n_ctx);
    Shared &sh = E.sh;
    const uint8_t *text = E.text;
    const bool streamed = E.streamed = !text && !o.host_parse && ntc::fastx_streamed_fastq(fx);
    // qualities, names and pairs exist only where the GPU parses the text: both of a pair's
    // inputs must reach it as text
    const auto text_only = [&](int mode, const TextOnly &t) {
        if (mode && o.host_parse)
            sh.fail(NTC_ERR_UNSUPPORTED, std::string(t.what) + ": host_parse = 1 parses on the host, which drops the " + t.lost);
        else if (mode && !text && !streamed)
            sh.fail(NTC_ERR_UNSUPPORTED, std::string(t.what) + ": the input is not FASTQ (" + t.not_fastq + ")");
    };
    text_only(q_mode, kQualText), text_only(n_mode, kNameText), text_only(pair_mode, kPairText);
    if (fo.mate_path && !(pair_mode && (o.host_parse || (!text && !streamed)))) {
        TextSrc *msrc = E.msrc;
        msrc[0].fx = fx;
        msrc[0].map = text;
        msrc[0].map_n = E.text_n;
        msrc[1].fx = fx2;
        msrc[1].map = ntc::fastx_mapped(fx2, &msrc[1].map_n);
        if (!msrc[1].map && !ntc::fastx_streamed_fastq(fx2))
            sh.fail(NTC_ERR_UNSUPPORTED, "pairs: the mate input is not FASTQ (mates are checked and woven in FASTQ text only)");
    }
    // the reader's gang: 8 threads copy + scan at ~45 GB/s on the box, as fast as 16 for the
    // pipeline and at less CPU beside the deflate pool (scripts/rt_sweep.sh); NTC_READ_THREADS
    // is the A/B hook
    const char *rt_env = std::getenv("NTC_READ_THREADS");
    E.RT = std::max(1, rt_env ? std::atoi(rt_env) : std::min(T, 8));
    if (text) {  // bytes per record from the first MiB
        const size_t m = (size_t)std::min<uint64_t>(E.text_n, 1u << 20);
        uint64_t nl = 0;
        for (size_t i = 0; i < m; i++) nl += text[i] == '\n';
        E.rec_bytes = nl >= 4 ? 4.0 * (double)m / (double)nl : (double)m + 1;
    }

    std::thread reader([&E] { E.read_batches(); });
    std::vector<std::thread> gpus, pool;
    for (int c = 0; c < n_ctx; c++) gpus.emplace_back([&E, c] { E.run_gpu(c); });
    for (int t = 0; t < T; t++) pool.emplace_back([&E] { E.deflate_worker(); });
    E.write_blocks();
    E.etrace("all written", 0);
    reader.join();
    for (auto &t : gpus) t.join();
    for (auto &t : pool) t.join();
    E.etrace("threads joined", 0);
    for (auto &kv : E.done) kv.second.free_parts();
    for (auto &b : ring) {
        pinned_free(b.bases);
        pinned_free(b.offs);
        pinned_free(b.text);
    }
    E.etrace("buffers freed", 0);
    ntc::InflateCounts ic;
    ntc::fastx_inflate_counts(fx, &ic);
    if (fx2) ntc::fastx_inflate_counts(fx2, &ic);
    ntc_fastx_close(fx);
    if (fx2) ntc_fastx_close(fx2);
    if (inflater) ih.destroy(inflater);
    if (stats.i) {
        *stats.i = ntc_i_stats{};
        stats.i->engine = (uint32_t)job.inflate_engine;
        stats.i->members = ic.members, stats.i->bytes = ic.bytes, stats.i->runs = ic.runs, stats.i->fallback_runs = ic.fallback_runs;
        stats.i->seconds = ic.seconds;
    }
    E.etrace("input closed", 0);
    const int result = sh.error == -1 ? NTC_OK : sh.error;
    S.alloc_s += E.t_pin.load();
    S.parse_s = E.t_parse.load();
    S.gpu_s = E.t_gpu.load();
    S.deflate_s = E.t_deflate.load();
    S.write_s = E.t_write.load();
    S.wall_s = secs(t0, Clock::now());
    S.threads = T;
    S.gpu_parsed = (int32_t)E.text_batches.load();
    S.bad_read = sh.bad_read;
    std::snprintf(S.error, sizeof(S.error), "%s", result == NTC_OK ? "" : sh.msg.c_str());
    ntc_p_stats PS{};
    PS.mode = (uint32_t)pair_mode;
    PS.pairs = pair_mode ? S.reads / 2 : 0;
    PS.bytes1 = E.msrc[0].sent;
    PS.bytes2 = E.msrc[1].sent;
    if (stats.pipe) *stats.pipe = S;
    if (stats.nx) *stats.nx = E.NX;
    if (stats.q) *stats.q = E.QS;
    if (stats.n) *stats.n = E.NS;
    if (stats.d) *stats.d = E.DS;
    if (stats.p) *stats.p = PS;
    return result;
}

extern "C" {

int ntc_encode_file(ntc_ctx *const *ctxs, int n_ctx, const char *in_path, int out_fd, const ntc_pipeline_opts *opts,
                    ntc_pipeline_stats *stats) {
    FileJob job(ctxs, n_ctx, in_path, out_fd, opts);
    return encode_file(job, {stats});
}

int ntc_encode_file_nx(ntc_ctx *const *ctxs, int n_ctx, const char *in_path, int out_fd, int policy, int nx_fd,
                       const ntc_pipeline_opts *opts, ntc_pipeline_stats *stats, ntc_nx_stats *nx) {
    if (policy < 0) return NTC_ERR_INVALID_ARG;
    FileJob job(ctxs, n_ctx, in_path, out_fd, opts);
    job.has_policy = true;
    job.fo.nx_policy = policy;
    job.fo.nx_fd = nx_fd;
    return encode_file(job, {stats, nx});
}

int ntc_encode_file_ex(ntc_ctx *const *ctxs, int n_ctx, const char *in_path, int out_fd, const ntc_file_opts *fo,
                       const ntc_pipeline_opts *opts, ntc_pipeline_stats *stats, ntc_nx_stats *nx, ntc_q_stats *q) {
    if (!fo || fo->nx_policy < 0) return NTC_ERR_INVALID_ARG;
    FileJob job(ctxs, n_ctx, in_path, out_fd, opts);
    job.take_ex(*fo);
    return encode_file(job, {stats, nx, q});
}

int ntc_encode_file_ex2(ntc_ctx *const *ctxs, int n_ctx, const char *in_path, int out_fd, const ntc_file_opts2 *fo,
                        const ntc_pipeline_opts *opts, ntc_pipeline_stats *stats, ntc_nx_stats *nx, ntc_q_stats *q,
                        ntc_n_stats *n) {
    if (!fo || fo->struct_bytes < sizeof(ntc_file_opts2) || fo->nx_policy < 0) return NTC_ERR_INVALID_ARG;
    FileJob job(ctxs, n_ctx, in_path, out_fd, opts);
    job.take_ex2(*fo);
    return encode_file(job, {stats, nx, q, n});
}

int ntc_encode_file_ex3(ntc_ctx *const *ctxs, int n_ctx, const char *in_path, int out_fd, const ntc_file_opts3 *fo,
                        const ntc_pipeline_opts *opts, ntc_pipeline_stats *stats, ntc_nx_stats *nx, ntc_q_stats *q,
                        ntc_n_stats *n, ntc_d_stats *d) {
    if (!fo || fo->struct_bytes < sizeof(ntc_file_opts3) || fo->nx_policy < 0) return NTC_ERR_INVALID_ARG;
    FileJob job(ctxs, n_ctx, in_path, out_fd, opts);
    job.take_ex3(*fo);
    return encode_file(job, {stats, nx, q, n, d});
}

int ntc_encode_file_ex4(ntc_ctx *const *ctxs, int n_ctx, const char *in_path, int out_fd, const ntc_file_opts4 *fo,
                        const ntc_pipeline_opts *opts, ntc_pipeline_stats *stats, ntc_nx_stats *nx, ntc_q_stats *q,
                        ntc_n_stats *n, ntc_d_stats *d, ntc_p_stats *p) {
    if (!fo || fo->struct_bytes < sizeof(ntc_file_opts4) || fo->nx_policy < 0) return NTC_ERR_INVALID_ARG;
    FileJob job(ctxs, n_ctx, in_path, out_fd, opts);
    job.fo = *fo;
    job.has_policy = true;
    return encode_file(job, {stats, nx, q, n, d, p});
}

int ntc_encode_file_ex6(ntc_ctx *const *ctxs, int n_ctx, const char *in_path, int out_fd, const ntc_file_opts6 *fo,
                        const ntc_pipeline_opts *opts, ntc_pipeline_stats *stats, ntc_nx_stats *nx, ntc_q_stats *q,
                        ntc_n_stats *n, ntc_d_stats *d, ntc_p_stats *p, ntc_i_stats *i) {
    if (!fo || fo->struct_bytes < sizeof(ntc_file_opts6) || fo->nx_policy < 0 || fo->reserved) return NTC_ERR_INVALID_ARG;
    FileJob job(ctxs, n_ctx, in_path, out_fd, opts);
    job.take_ex3(*fo);
    job.fo.pair_mode = fo->pair_mode, job.fo.mate_path = fo->mate_path, job.fo.out_fd2 = fo->out_fd2;
    job.inflate_engine = fo->inflate_engine;
    FileStats out{stats, nx, q, n, d, p};
    out.i = i;
    return encode_file(job, out);
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
//
// The stages are scan_extents and the member functions of Decoder (unzip_worker, run_gpu,
// assign_ahead, write_text), which holds what they share; ntc::pipe::decode_file checks the
// request, loads the side files and runs them.
// ---------------------------------------------------------------------------------------
namespace {

struct DBlock {
    uint64_t a, len;   // byte range of the block
    uint64_t n_recs;   // records (the flag stream's num_u64)
    uint64_t n_reads;  // reads (stream 0's num_records)
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
    uint64_t n_out = 0;      // reads in the text: n_reads, fewer where a range cuts the batch
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

// A side file read once into owned buffers: entry i belongs to block i of the file (the
// exception runs: to the read they name).  loaded: the call named the file.
template <class Entry>
struct SideFile {
    bool loaded = false;
    Entry *metas = nullptr;
    uint64_t n = 0, bytes = 0;
    uint8_t *payload = nullptr;
    int mode = 0;
    ~SideFile() {
        ntc_buffer_free(metas);
        ntc_buffer_free(payload);
    }
};
// a call that ends before its pipeline starts: only the reason in the stats
int refuse(int rc, ntc_pipeline_stats *stats, const std::string &why) {
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        stats->bad_read = -1;
        std::snprintf(stats->error, sizeof(stats->error), "%s", why.c_str());
    }
    return rc;
}
std::string side_file_error(const char *what, int rc) {
    return std::string(what) + ": " + (rc == NTC_ERR_IO ? "cannot read the side file" : "malformed side file");
}
// hands a context the sections of blocks [first, first + n), their payload from offset 0:
// set(metas, n, payload, bytes) wraps the hook
template <class Meta, class Set>
int put_sections(const SideFile<Meta> &f, uint64_t first, uint64_t n, std::vector<Meta> &tmp, const Set &set) {
    if (!f.loaded || n == 0) return NTC_OK;
    if (first + n > f.n) return NTC_ERR_FORMAT;
    tmp.assign(f.metas + first, f.metas + first + n);
    const uint64_t base = tmp[0].payload_off;
    for (auto &m : tmp) m.payload_off -= base;
    const uint64_t bytes = tmp.back().payload_off + tmp.back().payload_bytes;
    return set(tmp.data(), n, f.payload + base, bytes);
}

// decode: the streams decoded on the host pool instead of the GPU (NTC_HOST_UNPACK=1)
bool host_unpack_on() {
    const char *h = std::getenv("NTC_HOST_UNPACK");
    return h && std::atoi(h) > 0;
}

// ---- map + extents ------------------------------------------------------------------
// A block's buffers are sized from its headers before anything is inflated, so each
// header is checked against its own gzip stream first: the ISIZE trailer must equal
// 8 x encoded_size, which deflate cannot exceed 1032 x block_size, and stream 2 (Rice: one
// bit per value at least) bounds num_u64.  A block that fails is damaged -- the output ends
// before it, as the reference's loop ends at decode_block's Err (main.rs:202) -- instead of
// a pinned allocation sized from garbage.
std::vector<DBlock> scan_extents(const uint8_t *data, uint64_t fsize) {
    auto le32 = [&](uint64_t p) { return (uint64_t)data[p] | (uint64_t)data[p + 1] << 8 | (uint64_t)data[p + 2] << 16 |
                                         (uint64_t)data[p + 3] << 24; };
    std::vector<DBlock> blocks;
    for (uint64_t pos = 32; pos < fsize;) {  // after the 32-byte file header (main.rs:196-198)
        uint64_t p = pos, nrec = 0, nreads = 0, pay = 0;
        bool whole = true, bad = false;
        for (int s = 0; s < 4 && whole; s++) {
            if (p + 32 > fsize) {
                whole = false;
                break;
            }
            const uint64_t bs = le32(p), enc = le32(p + 12);
            if (s == 0) nreads = le32(p + 4);
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
        blocks.push_back(bad ? DBlock{pos, p - pos, 0, 0, 0, true} : DBlock{pos, p - pos, nrec, nreads, pay, false});
        pos = p;
    }
    return blocks;
}

struct Decoder {
    // ---- the request and the input (fixed before the threads start) ------------------------------
    ntc_ctx *const *ctxs;
    const int n_ctx;
    const int out_fd, out_fd2, pair_mode;
    const bool discard;  // out_fd -1: everything but the copy of the text off the device and its write
    const bool split;    // pairs: each batch's text comes back in two parts
    const bool bgzf;     // NTC_OUT_BGZF: each batch's text comes back as BGZF members (each part's, under pairs)
    SideFile<ntc_nx_run> nxf;  // the exception runs; each batch finds its own by its first read (put_runs)
    uint32_t nx_sub = 0;
    SideFile<ntc_qual_meta> qf;
    SideFile<ntc_name_meta> nf;
    SideFile<ntc_digest_meta> df;  // the expected digests
    const uint8_t *data = nullptr;
    uint64_t fsize = 0;
    std::vector<DBlock> blocks;  // the blocks to decode: all of the file, or those a range touches
    // a range of reads (ranged): blocks[0] is block blk_base of the file and of every side file;
    // head_skip / tail_skip reads of the first / last batch stay out of the text
    bool ranged = false;
    uint64_t blk_base = 0, head_skip = 0, tail_skip = 0;
    uint64_t bpb = 0, b0n = 0, n_batches = 0;
    int NB = 0;
    bool gpu_unpack = true;
    Clock::time_point t0;
    uint64_t trace_n = 0;
    // ---- shared by the threads, under sh.mu ----------------------------------------------------
    Shared sh;
    std::vector<DSlot> slots;
    uint64_t next_task = 0;    // next block to unzip
    uint64_t next_id = 1;      // main.rs:204: seq.{i+1}
    int64_t stop_batch = -1;   // batch holding the first damaged block (output ends in it)
    uint64_t next_assign = 0;  // next batch to number
    ntc_pipeline_stats S{};
    ntc_d_stats DS{};
    ntc_p_stats PS{};  // the writer's
    ntc_z_stats ZS{};  // the members of the batches decoded (under sh.mu)
    off_t out_pos = 0;
    bool seekable = false;
    std::atomic<double> t_unzip{0}, t_gpu{0}, t_write{0}, t_pin{0};

    Decoder(const FileJob &job, bool discard_)
        : ctxs(job.ctxs), n_ctx(job.n_ctx), out_fd(job.out_fd), out_fd2(job.fo.out_fd2), pair_mode(job.fo.pair_mode),
          discard(discard_), split(job.fo.pair_mode && !discard_), bgzf(job.out_format == NTC_OUT_BGZF && !discard_) {}

    uint64_t batch_first(uint64_t b) const { return b == 0 ? 0 : b0n + (b - 1) * bpb; }
    uint64_t batch_of(uint64_t blk) const { return blk < b0n ? 0 : 1 + (blk - b0n) / bpb; }
    uint64_t batch_end(uint64_t b) const { return std::min<uint64_t>(blocks.size(), batch_first(b + 1)); }
    DSlot &slot_of(uint64_t b) { return slots[(size_t)(b % (uint64_t)NB)]; }
    bool stopped_before(uint64_t b) const { return stop_batch >= 0 && (int64_t)b > stop_batch; }
    // NTC_PIPE_TRACE=n: the first n batches' events on stderr (ms from the call's start)
    void trace(const char *what, uint64_t b) const {
        if (b < trace_n) std::fprintf(stderr, "[pipe] %8.3f ms batch %llu %s\n", 1e3 * secs(t0, Clock::now()),
                                      (unsigned long long)b, what);
    }
    // the names' bytes of blocks [first, first + n) (those the side file has): room in the text
    uint64_t name_room(uint64_t first, uint64_t n) const {
        uint64_t bytes = 0;
        for (uint64_t k = first; nf.loaded && k < first + n && k < nf.n; k++) bytes += nf.metas[k].name_bytes;
        return bytes;
    }
    bool fail_ctx(int rc, int c) {
        sh.fail(rc, std::string("decode: ") + ntc_last_error(ctxs[c]));
        return false;
    }
    std::string place_range(uint64_t first, uint64_t count, ntc_r_stats &R);
    bool ensure_pinned(void **p, uint64_t *cap, uint64_t need);
    void prepin_first_batches();
    void assign_ahead();
    int put_runs(ntc_ctx *ctx, uint64_t first, uint64_t n, std::vector<ntc_nx_run> &tmp) const;
    void digest_verdict(ntc_ctx *ctx, int rc, uint64_t first, uint64_t n, uint64_t first_read, std::string &msg,
                        int64_t &bad_read);
    bool warm_up(int c);
    bool decode_batch(int c, uint64_t b, DSlot &sl, uint64_t nb, std::vector<ntc_nx_run> &nx_tmp,
                      std::vector<ntc_qual_meta> &q_tmp, std::vector<ntc_name_meta> &n_tmp);
    void run_gpu(int c);
    void unzip_worker();
    void write_text();
};

// Reads [first, first + count) of the file (blocks = all of its blocks, the side files loaded):
// keeps the blocks that hold them and sets the numbering's start and the reads to leave out at
// both ends; R gets the placement.  Returns why not, or "": "range: ..." a request the archive
// cannot serve (NTC_ERR_INVALID_ARG), "build: ..." a build without the window, anything else a
// file that cannot be trusted for it (NTC_ERR_FORMAT).  Only metadata is read.
std::string Decoder::place_range(uint64_t first, uint64_t count, ntc_r_stats &R) {
    char buf[200];
    uint64_t known = 0;  // reads of the blocks before the first bad one: only those have numbers
    uint64_t first_bad = blocks.size();
    for (uint64_t i = 0; i < blocks.size(); i++) {
        if (blocks[i].bad) {
            first_bad = i;
            break;
        }
        known += blocks[i].n_reads;
    }
    if (first >= R.reads_total || count > R.reads_total - first) {
        std::snprintf(buf, sizeof(buf), "range: reads %llu..%llu asked of an archive that holds %llu reads in %llu blocks",
                      (unsigned long long)first, (unsigned long long)(first + count - 1), (unsigned long long)R.reads_total,
                      (unsigned long long)blocks.size());
        return buf;
    }
    if (pair_mode && ((first | count) & 1)) return "range: under pairs the first read and the count must be even (whole pairs)";
    if (first + count > known) {
        std::snprintf(buf, sizeof(buf), "damaged block %llu at or before the range: the reads after it have no numbers",
                      (unsigned long long)first_bad);
        return buf;
    }
    // every given side file describes exactly these blocks
    const auto sections = [&](const char *what, bool loaded, uint64_t n, auto reads_of) -> std::string {
        if (!loaded) return "";
        if (n != blocks.size()) {
            std::snprintf(buf, sizeof(buf), "%s: %llu sections for %llu blocks (the side file belongs to another encoding)", what,
                          (unsigned long long)n, (unsigned long long)blocks.size());
            return buf;
        }
        for (uint64_t i = 0; i < n; i++)
            if (!blocks[i].bad && reads_of(i) != blocks[i].n_reads) {
                std::snprintf(buf, sizeof(buf), "%s: section %llu holds %llu reads, block %llu's header says %llu", what,
                              (unsigned long long)i, (unsigned long long)reads_of(i), (unsigned long long)i,
                              (unsigned long long)blocks[i].n_reads);
                return buf;
            }
        return "";
    };
    std::string why = sections("qualities", qf.loaded, qf.n, [&](uint64_t i) { return (uint64_t)qf.metas[i].n_reads; });
    if (why.empty()) why = sections("names", nf.loaded, nf.n, [&](uint64_t i) { return (uint64_t)nf.metas[i].n_reads; });
    if (why.empty()) why = sections("digests", df.loaded, df.n, [&](uint64_t i) { return (uint64_t)df.metas[i].n_reads; });
    if (!why.empty()) return why;
    uint64_t b0 = 0, before = 0;
    while (before + blocks[b0].n_reads <= first) before += blocks[b0++].n_reads;
    uint64_t b1 = b0, upto = before + blocks[b0].n_reads;  // reads of blocks [0, b1]
    while (upto < first + count) upto += blocks[++b1].n_reads;
    ranged = true;
    blk_base = b0;
    head_skip = first - before;
    tail_skip = upto - (first + count);
    if ((head_skip || tail_skip) && !ntc::g_w_hooks.decode_set_window) return "build: no text window in this build";
    next_id = 1 + before;
    blocks = std::vector<DBlock>(blocks.begin() + (std::ptrdiff_t)b0, blocks.begin() + (std::ptrdiff_t)b1 + 1);
    R.head_skipped = head_skip;
    R.tail_skipped = tail_skip;
    return "";
}

// pinned buffers are sized per batch (grown in the claiming thread, outside the lock)
bool Decoder::ensure_pinned(void **p, uint64_t *cap, uint64_t need) {
    if (need <= *cap) return true;
    const auto tp = Clock::now();
    pinned_free(*p);
    *p = nullptr;
    *cap = 0;
    const uint64_t want = need + need / 8 + 4096;
    if ((*p = pinned_alloc(want))) *cap = want;
    add_time(t_pin, secs(tp, Clock::now()));
    return *p != nullptr;
}

// ---- pinned buffers of the first batches, allocated in parallel -----------------------------
// (each is mapped, touched and registered: ~10 ms for a batch's 21 MB of text, which the
// first batch would otherwise wait for in turn; later batches reuse them).  The text size
// is a guess from the records (48 bytes each: C91's reads take 41); a batch that needs
// more regrows its buffer as before.
void Decoder::prepin_first_batches() {
    std::vector<std::thread> pre;
    for (uint64_t j = 0; j < (uint64_t)NB && j < n_batches; j++)
        pre.emplace_back([this, j] {
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

// ">seq.N" numbering: batch a gets first_id once every batch before it has its read count
// (host unpack: the batch is complete; GPU unpack: the device has decoded its streams).
// Whichever thread completes a count numbers the batches as far ahead as they allow, so
// their GPU work overlaps the writes of the batches before them (round 5's first version
// numbered them in the writer's loop only: a batch's text then waited for the write of
// the one before it, 3.1 ms per batch where the write takes 2).
void Decoder::assign_ahead() {  // under sh.mu
    while (next_assign < n_batches) {
        if (stopped_before(next_assign)) break;
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
}

// hands ctx the runs of reads [first, first + n) (file numbering), read relative to first
int Decoder::put_runs(ntc_ctx *ctx, uint64_t first, uint64_t n, std::vector<ntc_nx_run> &tmp) const {
    if (!nxf.n) return NTC_OK;
    const auto less = [](const ntc_nx_run &x, uint64_t v) { return x.read < v; };
    const ntc_nx_run *lo = std::lower_bound(nxf.metas, nxf.metas + nxf.n, first, less);
    const ntc_nx_run *hi = std::lower_bound(lo, (const ntc_nx_run *)(nxf.metas + nxf.n), first + n, less);
    tmp.assign(lo, hi);
    for (auto &r : tmp) r.read -= first;
    return ntc::g_nx_hooks.decode_set_exceptions(ctx, tmp.data(), tmp.size(), nx_sub);
}

// after a batch's decode call (rc): what it checked into the stats (under sh.mu), and for
// NTC_ERR_DIGEST the block in the file's numbering, its first read and the component
void Decoder::digest_verdict(ntc_ctx *ctx, int rc, uint64_t first, uint64_t n, uint64_t first_read, std::string &msg,
                             int64_t &bad_read) {
    if (!df.loaded || n == 0 || (rc != NTC_OK && rc != NTC_ERR_DIGEST)) return;
    std::vector<ntc_digest_meta> got(n);
    uint64_t have = 0;
    if (ntc::g_d_hooks.decode_digests(ctx, got.data(), n, &have) != NTC_OK || have != n) return;
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
}

// ---- GPU drivers ---------------------------------------------------------------------------
// While the pool inflates the first batches: one tiny unpack (an empty block) and
// one tiny decode (a one-base read), so the first real calls find the unpacker's
// and the formatter's code objects loaded (HIP loads them at a kernel's first
// launch: ~10 ms on the first batch's path otherwise)
bool Decoder::warm_up(int c) {
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
    return w3 ? fail_ctx(NTC_ERR_HIP, c) : true;
}

// Batch b (in sl, numbered, nb blocks of it to decode) on context c: room for its text, its
// side data handed to the context -- exception runs, quality and name sections, expected
// digests -- the decode call, the digests' verdict and the pair split.  false: failed (sh says
// why)
bool Decoder::decode_batch(int c, uint64_t b, DSlot &sl, uint64_t nb, std::vector<ntc_nx_run> &nx_tmp,
                           std::vector<ntc_qual_meta> &q_tmp, std::vector<ntc_name_meta> &n_tmp) {
    ntc_ctx *ctx = ctxs[c];
    const uint64_t q_per_base = qf.loaded ? 1 : 0, q_per_read = qf.loaded ? 3 : 0;  // FASTQ: "+\n", qualities, "\n" more
    const uint64_t need = sl.n_bases * (1 + q_per_base) + (7 + q_per_read) * sl.n_reads +
                          digits_total(sl.first_id, sl.n_reads) + name_room(blk_base + sl.first_block, nb) + 64;
    const auto tg = Clock::now();
    // (BGZF: the bound of the members of that much text, in up to two parts)
    if (!discard && !ensure_pinned((void **)&sl.text, &sl.cap_text, bgzf ? ntc::bgzf_bound(need) + 2 * ntc::kBgzfSlack : need)) {
        sh.fail(NTC_ERR_HIP, "pinned host allocation failed");
        return false;
    }
    if (const int rx = put_runs(ctx, sl.first_id - 1, sl.n_reads, nx_tmp)) return fail_ctx(rx, c);
    const char *what = "qualities: fewer sections than blocks, or a section that does not fit its block";
    int rx = put_sections(qf, blk_base + sl.first_block, nb, q_tmp,
                          [&](const ntc_qual_meta *m, uint64_t n, const uint8_t *p, uint64_t bytes) {
                              return ntc::g_q_hooks.decode_set_qualities(ctx, m, n, p, bytes);
                          });
    if (!rx) {
        what = "names: fewer sections than blocks, or a section that does not fit its block";
        rx = put_sections(nf, blk_base + sl.first_block, nb, n_tmp,
                          [&](const ntc_name_meta *m, uint64_t n, const uint8_t *p, uint64_t bytes) {
                              return ntc::g_n_hooks.decode_set_names(ctx, m, n, p, bytes);
                          });
    }
    if (!rx && df.loaded) {  // the expected digests of the blocks
        what = "digests: fewer sections than blocks";
        rx = blk_base + sl.first_block + nb > df.n
                 ? NTC_ERR_FORMAT
                 : ntc::g_d_hooks.decode_set_digests(ctx, df.metas + blk_base + sl.first_block, nb);
    }
    if (rx == NTC_ERR_FORMAT) {
        sh.fail(rx, what);
        return false;
    }
    if (rx) return fail_ctx(rx, c);
    sl.n_out = sl.n_reads;
    if (ranged) {
        // strict: every touched block decoded, to the read count its header gave (the range was
        // placed by those counts)
        uint64_t by_header = 0;
        for (uint64_t i = 0; i < sl.n_blocks; i++) by_header += blocks[sl.first_block + i].n_reads;
        if (nb != sl.n_blocks || by_header != sl.n_reads) {
            char why[160];
            if (nb != sl.n_blocks)
                std::snprintf(why, sizeof(why), "damaged block %llu inside the range", (unsigned long long)(blk_base + sl.first_block + nb));
            else
                std::snprintf(why, sizeof(why), "blocks %llu.. hold %llu reads, their headers say %llu: the range cannot be placed",
                              (unsigned long long)(blk_base + sl.first_block), (unsigned long long)sl.n_reads,
                              (unsigned long long)by_header);
            sh.fail(NTC_ERR_FORMAT, why);
            return false;
        }
        // the range's first and last batch: only its reads are formatted
        const uint64_t w0 = b == 0 ? head_skip : 0, w1 = sl.n_reads - (b + 1 == n_batches ? tail_skip : 0);
        sl.n_out = w1 - w0;
        if (sl.n_out != sl.n_reads && (rx = ntc::g_w_hooks.decode_set_window(ctx, w0, w1 - w0))) return fail_ctx(rx, c);
    }
    uint64_t len = 0;
    const uint64_t cap = discard ? 0 : sl.cap_text;
    const int rc = gpu_unpack ? ntc_decode_fasta_unpacked(ctx, sl.first_id, sl.text, cap, &len)
                              : ntc_decode_fasta(ctx, sl.recs, sl.n_recs, sl.n_reads, sl.n_bases, sl.first_id, sl.text, cap, &len);
    add_time(t_gpu, secs(tg, Clock::now()));
    if (rc) {
        std::string msg = std::string("decode: ") + ntc_last_error(ctx);
        int64_t bad = -1;
        digest_verdict(ctx, rc, blk_base + sl.first_block, nb, sl.first_id - 1, msg, bad);
        sh.fail(rc, msg, bad);
        return false;
    }
    uint64_t first = 0;
    if (split && ntc::g_p_hooks.pair_split(ctx, &first)) return fail_ctx(NTC_ERR_FORMAT, c);
    ntc_bgzf_counts zc{};
    if (bgzf && ntc::g_b_hooks.last_counts(ctx, &zc)) return fail_ctx(NTC_ERR_HIP, c);
    std::lock_guard<std::mutex> g(sh.mu);
    ZS.members += zc.members, ZS.text_bytes += zc.text_bytes, ZS.bytes += zc.bytes;
    ZS.chunks_stored += zc.chunks_stored, ZS.chunks_huffman += zc.chunks_huffman, ZS.chunks_matches += zc.chunks_matches;
    ZS.seconds += zc.seconds;
    {
        std::string unused;
        int64_t bad = -1;
        digest_verdict(ctx, NTC_OK, blk_base + sl.first_block, nb, sl.first_id - 1, unused, bad);
    }
    sl.first_len = first;
    sl.text_len = len;
    sl.decoded = true;
    trace("decoded", b);
    S.gpu_done_s = secs(t0, Clock::now());
    sh.cv.notify_all();
    return true;
}

// A batch is complete when all of its blocks are in (or every block before its first
// damaged one, once no task of it is still running).  assign_ahead fixes first_id in batch
// order.
void Decoder::run_gpu(int c) {
    if (gpu_unpack && !std::getenv("NTC_NO_WARM") && !warm_up(c)) return;
    // out_fd -1: the text stays on the device; pairs: every text call of this thread returns its
    // two parts (the context drops either option when this thread ends)
    ModeGuard discard_guard(ntc::g_d_hooks.set_discard, ctxs + c, discard ? 1 : 0, 1);
    if (discard_guard.rc()) return (void)fail_ctx(NTC_ERR_HIP, c);
    ModeGuard pairs_guard(ntc::g_p_hooks.set_mode, ctxs + c, split ? 1 : 0, pair_mode);
    if (pairs_guard.rc()) return (void)fail_ctx(NTC_ERR_HIP, c);
    ModeGuard bgzf_guard(ntc::g_b_hooks.set_mode, ctxs + c, bgzf ? 1 : 0, 1);
    if (bgzf_guard.rc()) return (void)fail_ctx(NTC_ERR_HIP, c);
    std::vector<ntc_nx_run> nx_tmp;  // a batch's exception runs, renumbered from its first read
    std::vector<ntc_qual_meta> q_tmp;  // ... and its quality sections
    std::vector<ntc_name_meta> n_tmp;  // ... and its name sections
    for (uint64_t b = (uint64_t)c;; b += (uint64_t)n_ctx) {
        DSlot *slp;
        {
            // GPU unpack: the batch's streams are decoded on the device as soon as every block of
            // it is inflated (or found damaged); host unpack: the batch waits for its numbering
            std::unique_lock<std::mutex> g(sh.mu);
            sh.cv.wait(g, [&] {
                return sh.error != NTC_OK || b >= n_batches || stopped_before(b) ||
                       (slot_of(b).batch == b && (gpu_unpack ? slot_of(b).finished == slot_of(b).n_blocks : slot_of(b).ready));
            });
            if (sh.error != NTC_OK || b >= n_batches || stopped_before(b)) return;
            slp = &slot_of(b);
        }
        DSlot &sl = *slp;
        const uint64_t nb = sl.bad_block >= 0 ? (uint64_t)sl.bad_block : sl.n_blocks;  // the blocks before a damaged one
        if (gpu_unpack) {  // its read count numbers the batches after it
            const auto tg = Clock::now();
            uint64_t ok = 0, nr = 0, nbs = 0;
            const int rc = ntc_unpack_streams(ctxs[c], sl.pay, sl.n_pay, sl.metas.data(), nb, &ok, &nr, &nbs);
            add_time(t_gpu, secs(tg, Clock::now()));
            if (rc) return (void)fail_ctx(rc, c);
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
        if (!decode_batch(c, b, sl, nb, nx_tmp, q_tmp, n_tmp)) return;
    }
}

// ---- unzip pool ------------------------------------------------------------------------
// Blocks are taken in file order; the first block of a batch claims the batch's slot
// (free once the writer is done with batch b - NB) and sizes its record buffer.  Past a
// damaged block no later batch is started; the rest of its own batch is still unzipped
// so that the batch completes (only the blocks before the damaged one are decoded).
void Decoder::unzip_worker() {
    for (;;) {
        uint64_t blk, b;
        bool first;
        {
            std::unique_lock<std::mutex> g(sh.mu);
            auto exhausted = [&] {
                return sh.error != NTC_OK || next_task >= blocks.size() || stopped_before(batch_of(next_task));
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
}

// ---- assigner + writer (the calling thread) ------------------------------------------------------
void Decoder::write_text() {
    struct stat ost;
    // pwrite only into a regular file opened without O_APPEND (Linux pwrite ignores the
    // offset under O_APPEND); the shared file offset is moved past the text at the end, so
    // `{ decode a; decode b; } > out` keeps both outputs as the reference's stdout does
    const int fl = fcntl(out_fd, F_GETFL);
    seekable = fstat(out_fd, &ost) == 0 && S_ISREG(ost.st_mode) && fl >= 0 && !(fl & O_APPEND) &&
               lseek(out_fd, 0, SEEK_CUR) >= 0;
    out_pos = seekable ? lseek(out_fd, 0, SEEK_CUR) : 0;
    // one writer: buffered writes into one file serialise on its inode lock, and on the GPU
    // box one thread's pwrite put 1.6 GB into the page cache at 12.6 GB/s against 10.4 from
    // 8 threads at their own offsets and 1.9 through a shared mapping
    // (profiles/round5/write_bw_box.jsonl, scripts/write_bw.cpp)
    auto write_out = [&](const uint8_t *p, uint64_t n) -> bool {
        while (n) {
            const ssize_t w = seekable ? ::pwrite(out_fd, p, n, out_pos) : ::write(out_fd, p, n);
            if (w <= 0) return false;
            p += w;
            n -= (uint64_t)w;
            out_pos += w;
        }
        return true;
    };
    for (uint64_t b = 0; b < n_batches; b++) {
        DSlot *slp;
        {
            std::unique_lock<std::mutex> g(sh.mu);
            sh.cv.wait(g, [&] {
                if (sh.error != NTC_OK) return true;
                if (stopped_before(b)) return true;
                assign_ahead();
                const DSlot &sl = slot_of(b);
                return sl.batch == b && sl.decoded;
            });
            if (sh.error != NTC_OK || stopped_before(b)) break;
            slp = &slot_of(b);
        }
        const auto tw = Clock::now();
        if (split) {  // the mate-1 records to out_fd, the mate-2 records to out_fd2
            const uint64_t f = std::min(slp->first_len, slp->text_len);
            if (!write_out(slp->text, f) || !write_fd(out_fd2, slp->text + f, slp->text_len - f)) sh.fail(NTC_ERR_IO, "write failed");
            PS.bytes1 += f;
            PS.bytes2 += slp->text_len - f;
            PS.pairs += slp->n_out / 2;
        } else if (!discard && !write_out(slp->text, slp->text_len)) {
            sh.fail(NTC_ERR_IO, "write failed");
        }
        add_time(t_write, secs(tw, Clock::now()));
        std::lock_guard<std::mutex> g(sh.mu);
        if (b == 0) S.first_batch_s = secs(t0, Clock::now());
        trace("written", b);
        S.reads += slp->n_out;
        S.bases += slp->n_bases;
        S.bytes_out += slp->text_len;
        S.blocks += slp->bad_block >= 0 ? (uint64_t)slp->bad_block : slp->n_blocks;
        const bool last = stop_batch >= 0 && (int64_t)b == stop_batch;
        slp->batch = ~0ULL;  // free the slot
        sh.cv.notify_all();
        if (last) break;
    }
    std::lock_guard<std::mutex> g(sh.mu);
    if (sh.error == NTC_OK) sh.error = -1;  // stop the workers
    sh.cv.notify_all();
}

}  // namespace

int ntc::pipe::decode_file(const FileJob &job, const FileStats &stats) {
    ntc_ctx *const *ctxs = job.ctxs;
    const int n_ctx = job.n_ctx, out_fd = job.out_fd, pair_mode = job.fo.pair_mode, out_fd2 = job.fo.out_fd2;
    const char *nx_path = job.fo.nx_path, *q_path = job.fo.q_path, *n_path = job.fo.n_path, *d_path = job.fo.d_path;
    const bool discard = job.may_discard && out_fd == -1;
    if (!ctxs || n_ctx <= 0 || !job.in_path || (out_fd < 0 && !discard)) return NTC_ERR_INVALID_ARG;
    // pairs: the mate-1 records of each batch go to out_fd and its mate-2 records to out_fd2
    if (pair_mode < 0 || pair_mode > 2 || (pair_mode ? out_fd2 < 0 && !discard : out_fd2 != -1)) return NTC_ERR_INVALID_ARG;
    const ntc::PHooks &ph = ntc::g_p_hooks;
    if (pair_mode && (!ph.set_mode || !ph.pair_split)) return NTC_ERR_UNSUPPORTED;
    if (job.out_format != NTC_OUT_TEXT && job.out_format != NTC_OUT_BGZF) return NTC_ERR_INVALID_ARG;
    if (job.out_format == NTC_OUT_BGZF && (!ntc::g_b_hooks.set_mode || !ntc::g_b_hooks.last_counts)) return NTC_ERR_UNSUPPORTED;
    for (int i = 0; i < n_ctx; i++)
        if (!ctxs[i]) return NTC_ERR_INVALID_ARG;
    Decoder D(job, discard);
    D.ZS.out_format = (uint32_t)job.out_format;
    D.PS.mode = (uint32_t)pair_mode;
    // the side files, each read once
    if ((D.nxf.loaded = nx_path != nullptr)) {
        if (!ntc::g_nx_hooks.decode_set_exceptions) return NTC_ERR_UNSUPPORTED;
        if (const int r = ntc_nx_read(nx_path, &D.nxf.metas, &D.nxf.n, &D.nx_sub))
            return refuse(r, stats.pipe, side_file_error("exceptions", r));
    }
    if ((D.qf.loaded = q_path != nullptr)) {
        if (!ntc::g_q_hooks.decode_set_qualities) return NTC_ERR_UNSUPPORTED;
        if (const int r = ntc_q_read(q_path, &D.qf.mode, &D.qf.metas, &D.qf.n, &D.qf.payload, &D.qf.bytes))
            return refuse(r, stats.pipe, side_file_error("qualities", r));
    }
    if ((D.nf.loaded = n_path != nullptr)) {
        if (!ntc::g_n_hooks.decode_set_names) return NTC_ERR_UNSUPPORTED;
        if (const int r = ntc_n_read(n_path, &D.nf.mode, &D.nf.metas, &D.nf.n, &D.nf.payload, &D.nf.bytes))
            return refuse(r, stats.pipe, side_file_error("names", r));
    }
    const ntc::DHooks &dh = ntc::g_d_hooks;
    if (discard && !dh.set_discard) return NTC_ERR_UNSUPPORTED;
    if ((D.df.loaded = d_path != nullptr)) {  // the file names the index it was written against
        if (!dh.decode_set_digests || !dh.decode_digests || !dh.index_info) return NTC_ERR_UNSUPPORTED;
        uint64_t f_nodes = 0, nodes = 0;
        uint32_t f_components = 0, f_k = 0, k = 0;
        if (const int r = ntc_d_read(d_path, &f_components, &f_k, &f_nodes, &D.df.metas, &D.df.n))
            return refuse(r, stats.pipe, side_file_error("digests", r));
        if (const int r = dh.index_info(ctxs[0], &nodes, &k)) return refuse(r, stats.pipe, "digests: no index uploaded");
        if (k != f_k || nodes != f_nodes) {
            char why[200];
            std::snprintf(why, sizeof(why), "digests: the file was written against another index (k = %u, %llu nodes; "
                          "the index uploaded has k = %u, %llu nodes)", f_k, (unsigned long long)f_nodes, k,
                          (unsigned long long)nodes);
            return refuse(NTC_ERR_DIGEST, stats.pipe, why);
        }
    }
    ntc_pipeline_opts o{};
    if (job.opts) o = *job.opts;
    const int T = o.threads > 0 ? o.threads : ntc_host_threads();
    // two blocks per GPU call: ~21 MB of text per batch keeps the pinned ring small and the
    // writer (the bound: ~8 GB/s into one file's page cache) busy from the first 20 ms
    const uint64_t bpb = D.bpb = (uint64_t)(o.blocks_per_batch > 0 ? o.blocks_per_batch : 2);
    ntc_pipeline_stats &S = D.S;
    const auto t0 = D.t0 = Clock::now();

    const int fd = ::open(job.in_path, O_RDONLY);
    if (fd < 0) return NTC_ERR_IO;
    struct stat st;
    if (fstat(fd, &st) != 0) {
        ::close(fd);
        return NTC_ERR_IO;
    }
    const uint64_t fsize = D.fsize = (uint64_t)st.st_size;
    if (fsize) {
        D.data = (const uint8_t *)mmap(nullptr, fsize, PROT_READ, MAP_PRIVATE, fd, 0);
        if (D.data == MAP_FAILED) {
            ::close(fd);
            return NTC_ERR_IO;
        }
        madvise((void *)D.data, fsize, MADV_SEQUENTIAL);
    }
    ::close(fd);
    D.blocks = scan_extents(D.data, fsize);
    const uint64_t total_blocks = D.blocks.size();
    const bool clean_end = D.blocks.empty() ? fsize <= 32 : D.blocks.back().a + D.blocks.back().len == fsize;
    ntc_r_stats R{};
    R.blocks_total = total_blocks;
    for (const DBlock &db : D.blocks) R.reads_total += db.n_reads;
    if (job.read_count) {  // a range: only the blocks that hold it are kept (or the call is refused here)
        const std::string why = D.place_range(job.read_first, job.read_count, R);
        if (!why.empty()) {
            if (D.data) munmap((void *)D.data, fsize);
            if (stats.r) *stats.r = R;  // (what the archive holds, for the caller's message)
            const bool arg = why.compare(0, 6, "range:") == 0;
            return refuse(arg ? NTC_ERR_INVALID_ARG : why.compare(0, 6, "build:") == 0 ? NTC_ERR_UNSUPPORTED : NTC_ERR_FORMAT,
                          stats.pipe, why);
        }
    }
    const std::vector<DBlock> &blocks = D.blocks;
    // NTC_FIRST_BATCH_BLOCKS=n: batch 0 holds n blocks, the others blocks_per_batch.  A
    // one-block first batch (the writer -- the pipeline's bound -- starting sooner) measured
    // no better on the box: the first write still came at ~20 ms, pipeline 0.160-0.198 s
    // against 0.166-0.178 s (profiles/round6/e2e_first_batch/), so the default stays bpb.
    const char *fbe = std::getenv("NTC_FIRST_BATCH_BLOCKS");
    D.b0n = std::max<uint64_t>(1, std::min<uint64_t>(bpb, fbe ? (uint64_t)std::atoll(fbe) : bpb));
    D.n_batches = blocks.empty() ? 0 : D.batch_of(blocks.size() - 1) + 1;
    S.alloc_s = secs(t0, Clock::now());

    D.NB = n_ctx + 2;
    D.slots.resize((size_t)D.NB);
    // the streams decoded on the GPU (default) or on the host pool (NTC_HOST_UNPACK=1): the
    // 10 M-read decode pipeline ran at 8.0 against 7.6 Gbases/s on one MI355X box, the pool's
    // thread-time 0.11 against 0.64 s (profiles/round5/e2e_dec_*)
    D.gpu_unpack = !host_unpack_on();
    const char *tr = std::getenv("NTC_PIPE_TRACE");
    D.trace_n = tr ? (uint64_t)std::atoll(tr) : 0;
    Shared &sh = D.sh;

    std::vector<std::thread> gpus, pool;
    for (int c = 0; c < n_ctx; c++) gpus.emplace_back([&D, c] { D.run_gpu(c); });
    D.prepin_first_batches();
    for (int t = 0; t < T; t++) pool.emplace_back([&D] { D.unzip_worker(); });
    D.write_text();
    for (auto &t : pool) t.join();
    for (auto &t : gpus) t.join();
    for (auto &sl : D.slots) {
        pinned_free(sl.recs);
        pinned_free(sl.pay);
        pinned_free(sl.text);
    }
    if (D.data) munmap((void *)D.data, fsize);
    int result = sh.error == -1 ? NTC_OK : sh.error;
    const int64_t stop_batch = D.stop_batch;
    char damaged[120];
    std::snprintf(damaged, sizeof(damaged), "damaged block %llu: the output ends before it",
                  (unsigned long long)(D.blk_base + S.blocks));
    const auto wrong = [&](bool cond, const char *why) {  // an ending that turns a clean run into NTC_ERR_FORMAT
        if (result != NTC_OK || !cond) return;
        result = NTC_ERR_FORMAT;
        sh.msg = why;
    };
    // every batch checked its own runs; one past the file's last read belongs to another encoding
    wrong(!D.ranged && stop_batch < 0 && D.nxf.n && D.nxf.metas[D.nxf.n - 1].read >= S.reads,
          "exceptions: a run past the last read (the side file belongs to another encoding)");
    // an input that ended cleanly used exactly all sections
    wrong(stop_batch < 0 && clean_end && q_path && D.qf.n != total_blocks,
          "qualities: more sections than blocks (the side file belongs to another encoding)");
    wrong(stop_batch < 0 && clean_end && n_path && D.nf.n != total_blocks,
          "names: more sections than blocks (the side file belongs to another encoding)");
    // under a digest file the lenient endings are errors: the file is known not to be whole
    // (a range is as strict about the blocks it touches; it never reaches a truncated tail)
    wrong((d_path || D.ranged) && stop_batch >= 0, damaged);
    wrong(d_path && !D.ranged && !clean_end, "truncated input: the file ends inside a block");
    wrong(d_path && D.df.n != total_blocks,
          "digests: more sections than blocks (the input is truncated, or the side file belongs to another encoding)");
    // BGZF: the EOF member ends each output of a call that succeeded, and only of such a call
    if (D.bgzf && result == NTC_OK) {
        const uint8_t *eof = ntc::kBgzfEof;
        const uint64_t ne = sizeof(ntc::kBgzfEof);
        const bool ok1 = D.seekable ? ::pwrite(out_fd, eof, ne, D.out_pos) == (ssize_t)ne : write_fd(out_fd, eof, ne);
        const bool ok2 = !D.split || write_fd(out_fd2, eof, ne);
        if (!ok1 || !ok2) {
            result = NTC_ERR_IO;
            sh.msg = "write failed";
        } else {
            D.out_pos += (off_t)ne;
            S.bytes_out += ne * (D.split ? 2 : 1);
            if (D.split) D.PS.bytes1 += ne, D.PS.bytes2 += ne;
        }
    }
    if (D.seekable) (void)lseek(out_fd, D.out_pos, SEEK_SET);
    S.dropped_blocks = blocks.size() - S.blocks;  // after a damaged block (or none)
    S.alloc_s += D.t_pin.load();
    S.parse_s = D.t_unzip.load();
    S.gpu_s = D.t_gpu.load();
    S.write_s = D.t_write.load();
    S.wall_s = secs(t0, Clock::now());
    S.threads = T;
    S.bad_read = result == NTC_ERR_DIGEST ? sh.bad_read : -1;
    if (stats.d) *stats.d = D.DS;
    if (pair_mode && discard) D.PS.pairs = S.reads / 2;
    if (stats.p) *stats.p = D.PS;
    if (stats.z) *stats.z = D.ZS;
    R.first_block = D.blk_base;
    R.blocks_read = S.blocks;
    R.reads_written = S.reads;
    if (stats.r) *stats.r = R;
    if (result != NTC_OK)
        std::snprintf(S.error, sizeof(S.error), "%s", sh.msg.c_str());
    else if (stop_batch >= 0)  // not an error for the reference either: its loop just ends
        std::snprintf(S.error, sizeof(S.error), "damaged block %llu: output ends before it",
                      (unsigned long long)S.blocks);
    if (stats.pipe) *stats.pipe = S;
    return result;
}

extern "C" {

int ntc_decode_file(ntc_ctx *const *ctxs, int n_ctx, const char *in_path, int out_fd, const ntc_pipeline_opts *opts,
                    ntc_pipeline_stats *stats) {
    FileJob job(ctxs, n_ctx, in_path, out_fd, opts);
    return decode_file(job, {stats});
}

int ntc_decode_file_nx(ntc_ctx *const *ctxs, int n_ctx, const char *in_path, const char *nx_path, int out_fd,
                       const ntc_pipeline_opts *opts, ntc_pipeline_stats *stats) {
    FileJob job(ctxs, n_ctx, in_path, out_fd, opts);
    job.fo.nx_path = nx_path;
    return decode_file(job, {stats});
}

int ntc_decode_file_ex(ntc_ctx *const *ctxs, int n_ctx, const char *in_path, int out_fd, const ntc_file_opts *fo,
                       const ntc_pipeline_opts *opts, ntc_pipeline_stats *stats) {
    if (!fo) return NTC_ERR_INVALID_ARG;
    FileJob job(ctxs, n_ctx, in_path, out_fd, opts);
    job.take_ex(*fo);
    return decode_file(job, {stats});
}

int ntc_decode_file_ex2(ntc_ctx *const *ctxs, int n_ctx, const char *in_path, int out_fd, const ntc_file_opts2 *fo,
                        const ntc_pipeline_opts *opts, ntc_pipeline_stats *stats) {
    if (!fo || fo->struct_bytes < sizeof(ntc_file_opts2)) return NTC_ERR_INVALID_ARG;
    FileJob job(ctxs, n_ctx, in_path, out_fd, opts);
    job.take_ex2(*fo);
    return decode_file(job, {stats});
}

int ntc_decode_file_ex3(ntc_ctx *const *ctxs, int n_ctx, const char *in_path, int out_fd, const ntc_file_opts3 *fo,
                        const ntc_pipeline_opts *opts, ntc_pipeline_stats *stats, ntc_d_stats *d) {
    if (!fo || fo->struct_bytes < sizeof(ntc_file_opts3)) return NTC_ERR_INVALID_ARG;
    FileJob job(ctxs, n_ctx, in_path, out_fd, opts);
    job.take_ex3(*fo);
    job.may_discard = true;
    FileStats out{stats};
    out.d = d;
    return decode_file(job, out);
}

int ntc_decode_file_ex4(ntc_ctx *const *ctxs, int n_ctx, const char *in_path, int out_fd, const ntc_file_opts4 *fo,
                        const ntc_pipeline_opts *opts, ntc_pipeline_stats *stats, ntc_d_stats *d, ntc_p_stats *p) {
    if (!fo || fo->struct_bytes < sizeof(ntc_file_opts4)) return NTC_ERR_INVALID_ARG;
    FileJob job(ctxs, n_ctx, in_path, out_fd, opts);
    job.fo = *fo;
    job.may_discard = true;
    FileStats out{stats};
    out.d = d, out.p = p;
    return decode_file(job, out);
}

int ntc_decode_file_ex5(ntc_ctx *const *ctxs, int n_ctx, const char *in_path, int out_fd, const ntc_file_opts5 *fo,
                        const ntc_pipeline_opts *opts, ntc_pipeline_stats *stats, ntc_d_stats *d, ntc_p_stats *p,
                        ntc_r_stats *r) {
    if (!fo || fo->struct_bytes < sizeof(ntc_file_opts5)) return NTC_ERR_INVALID_ARG;
    FileJob job(ctxs, n_ctx, in_path, out_fd, opts);
    job.take_ex3(*fo);
    job.fo.pair_mode = fo->pair_mode, job.fo.mate_path = fo->mate_path, job.fo.out_fd2 = fo->out_fd2;
    job.may_discard = true;
    job.read_first = fo->read_first, job.read_count = fo->read_count;
    FileStats out{stats};
    out.d = d, out.p = p, out.r = r;
    return decode_file(job, out);
}

int ntc_decode_file_ex7(ntc_ctx *const *ctxs, int n_ctx, const char *in_path, int out_fd, const ntc_file_opts7 *fo,
                        const ntc_pipeline_opts *opts, ntc_pipeline_stats *stats, ntc_d_stats *d, ntc_p_stats *p,
                        ntc_r_stats *r, ntc_z_stats *z) {
    if (!fo || fo->struct_bytes < sizeof(ntc_file_opts7) || fo->reserved2) return NTC_ERR_INVALID_ARG;
    FileJob job(ctxs, n_ctx, in_path, out_fd, opts);
    job.take_ex3(*fo);
    job.fo.pair_mode = fo->pair_mode, job.fo.mate_path = fo->mate_path, job.fo.out_fd2 = fo->out_fd2;
    job.may_discard = true;
    job.read_first = fo->read_first, job.read_count = fo->read_count;
    job.out_format = fo->out_format;
    FileStats out{stats};
    out.d = d, out.p = p, out.r = r, out.z = z;
    return decode_file(job, out);
}

int ntc_archive_info(const char *path, ntc_archive_block **blocks, uint64_t *n_blocks, uint64_t *n_reads,
                     uint64_t *n_records, uint64_t *tail_bytes) {
    if (!path || !blocks) return NTC_ERR_INVALID_ARG;
    *blocks = nullptr;
    uint64_t nb = 0, reads = 0, recs = 0, tail = 0;
    const int fd = ::open(path, O_RDONLY);
    if (fd < 0) return NTC_ERR_IO;
    struct stat st;
    if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) {
        ::close(fd);
        return NTC_ERR_IO;
    }
    const uint64_t fsize = (uint64_t)st.st_size;
    if (fsize) {
        const uint8_t *data = (const uint8_t *)mmap(nullptr, fsize, PROT_READ, MAP_PRIVATE, fd, 0);
        if (data == MAP_FAILED) {
            ::close(fd);
            return NTC_ERR_IO;
        }
        const std::vector<DBlock> found = scan_extents(data, fsize);  // (the headers and each stream's gzip trailer: nothing is inflated)
        munmap((void *)data, fsize);
        nb = found.size();
        tail = fsize <= 32 ? 0 : fsize - (found.empty() ? 32 : found.back().a + found.back().len);
        if (nb && !(*blocks = (ntc_archive_block *)std::calloc(nb, sizeof(ntc_archive_block)))) {
            ::close(fd);
            return NTC_ERR_IO;
        }
        for (uint64_t i = 0; i < nb; i++) {
            (*blocks)[i] = ntc_archive_block{found[i].a, found[i].len, found[i].n_reads, found[i].n_recs, found[i].bad ? 1u : 0u, 0};
            reads += found[i].n_reads;
            recs += found[i].n_recs;
        }
    }
    ::close(fd);
    if (n_blocks) *n_blocks = nb;
    if (n_reads) *n_reads = reads;
    if (n_records) *n_records = recs;
    if (tail_bytes) *tail_bytes = tail;
    return NTC_OK;
}

}  // extern "C"
