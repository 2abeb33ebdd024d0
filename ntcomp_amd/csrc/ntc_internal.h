// Host-side internal types shared by the builder, index I/O and the C ABI.
#pragma once
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace ntc {

// SBWT subset matrix + LCS in host memory (the form kbo::build / load_sbwt hand over).
struct HostIndex {
    uint64_t n = 0;
    uint32_t k = 0;
    std::vector<uint64_t> rows[4];  // ceil(n/64) words each, LSB-first
    uint64_t C[4] = {0, 0, 0, 0};
    std::vector<uint8_t> lcs;       // n bytes
    // -p/--prefix-precalc lookup table (sbwt PrefixLookupTable): [start, end) per p-mer
    uint32_t prefix_len = 0;
    std::vector<uint64_t> prefix_ranges;  // 2 * 4^prefix_len words
};
// colex interval of every p-mer, first character most significant (index_io.cpp)
void prefix_table(const HostIndex &ix, uint32_t p, std::vector<uint64_t> &ranges);

void build_index(const uint8_t *seqs, const uint64_t *offs, uint64_t nseqs, uint32_t k,
                 bool revcomp, int threads, HostIndex &out);
bool save_index(const HostIndex &ix, const std::string &prefix, std::string &err);
bool load_index(const std::string &prefix, HostIndex &ix, std::string &err);  // either layout
enum { kIndexOwn = 0, kIndexSbwtRs = 1 };  // ntc_index_save_as layouts (index_io.cpp)
bool save_index_as(const HostIndex &ix, const std::string &prefix, int layout, std::string &err);

// T - 1 helper threads that run one job at a time together with the caller (pipeline.cpp:
// the reader's copy + scan of each batch; pgzip.cpp: the symbol conversion of each read;
// spawning threads per batch costs ~1 ms a batch): run(f) calls f(t) on every thread,
// t = 0 the caller, and returns when all are done.
struct Gang {
    std::mutex mu;
    std::condition_variable go, done;
    std::function<void(int)> job;
    uint64_t gen = 0;
    int running = 0;
    bool stop = false;
    std::vector<std::thread> th;
    explicit Gang(int T) {
        for (int t = 1; t < T; t++)
            th.emplace_back([this, t] {
                uint64_t seen = 0;
                for (;;) {
                    std::function<void(int)> j;
                    {
                        std::unique_lock<std::mutex> g(mu);
                        go.wait(g, [&] { return stop || gen != seen; });
                        if (stop) return;
                        seen = gen;
                        j = job;
                    }
                    j(t);
                    std::lock_guard<std::mutex> g(mu);
                    if (--running == 0) done.notify_all();
                }
            });
    }
    int size() const { return (int)th.size() + 1; }
    void run(const std::function<void(int)> &f) {
        {
            std::lock_guard<std::mutex> g(mu);
            job = f;
            running = (int)th.size();
            gen++;
        }
        go.notify_all();
        f(0);
        std::unique_lock<std::mutex> g(mu);
        done.wait(g, [&] { return running == 0; });
    }
    ~Gang() {
        {
            std::lock_guard<std::mutex> g(mu);
            stop = true;
        }
        go.notify_all();
        for (auto &x : th) x.join();
    }
};

}  // namespace ntc

struct ntc_fastx;
struct ntc_block_meta;
struct ntc_ctx;
struct ntc_nx_run;
struct ntc_qual_meta;
struct ntc_name_meta;
struct ntc_digest_meta;
struct ntc_inflate_member;
struct ntc_bgzf_counts;
namespace ntc {
// a plain FASTQ that ntc_fastx_open mapped: its bytes (null for any other input), and
// moving the mapped parser to byte pos (a record start) -- pipeline.cpp's GPU-parse reader
const uint8_t *fastx_mapped(ntc_fastx *fx, uint64_t *size);
void fastx_seek_mapped(ntc_fastx *fx, uint64_t pos);
// a FASTQ read through a decoder (gzip, BGZF, bz2, xz, zstd) or a pipe: the next decoded
// bytes into dst (up to cap; fewer only at the end of input), and bytes handed back so the
// host parser goes on from them (the GPU-parse reader's fallback)
bool fastx_streamed_fastq(ntc_fastx *fx);
uint64_t fastx_stream_read(ntc_fastx *fx, uint8_t *dst, uint64_t cap, bool *io_error);
void fastx_stream_unread(ntc_fastx *fx, const uint8_t *src, uint64_t n);

// Parallel inflate of a non-BGZF gzip file (pgzip.cpp): null when the file is not gzip.
// pgz_read: cap bytes into dst (fewer only at the end), 1 filled, 0 the end, -1 an error
// (corrupt or truncated data, a CRC or ISIZE mismatch).
// the GPU unpacker's block decode on the host (block_codec.cpp; the sanitizer stand-in)
int unpack_block_host(const ::ntc_block_meta &m, const uint8_t *payload, std::vector<uint64_t> &recs);
// The decode pipeline's device workspaces sized ahead for a batch of about n_recs records in
// pay_bytes of inflated streams (capi.cpp): hipMalloc'd while the first batch inflates
// rather than on its path.  Estimates: at most 3 values and one read per record, 48 bytes of
// FASTA per record; a batch that needs more grows them as before.  host (pinned, host_bytes)
// takes one copy each way of up to 4 MiB: the process's first large copies start the DMA
// engines (7.7 ms before the first batch's text came back otherwise).
int reserve_decode(::ntc_ctx *ctx, uint64_t pay_bytes, uint64_t n_recs, uint8_t *host, uint64_t host_bytes);
// The GPU stage's non-ACGT entry points as the pipelines reach them (pipeline.cpp defines
// the table, all null; capi.cpp fills it when the library loads).  A build of pipeline.cpp
// without capi.cpp -- the sanitizer build over tests/san/gpu_stub.cpp -- links without them,
// and ntc_encode_file_nx / ntc_decode_file_nx then answer NTC_ERR_UNSUPPORTED to a policy
// other than error or to a side file.
struct NxHooks {
    int (*set_policy)(::ntc_ctx *ctx, int policy);                      // ctx option "non_acgt"
    int (*last_counts)(::ntc_ctx *ctx, uint32_t *sub, uint64_t *runs, uint64_t *bases);  // "nx_sub", "nx_runs", "nx_bases"
    int (*encode_exceptions)(::ntc_ctx *ctx, ::ntc_nx_run *out, uint64_t capacity, uint64_t *n_runs);
    int (*decode_set_exceptions)(::ntc_ctx *ctx, const ::ntc_nx_run *runs, uint64_t n_runs, uint32_t sub);
};
extern NxHooks g_nx_hooks;
// The same for quality scores: with the table null, ntc_encode_file_ex / ntc_decode_file_ex
// answer NTC_ERR_UNSUPPORTED to a quality mode other than drop or to a quality file.
struct QHooks {
    int (*set_mode)(::ntc_ctx *ctx, int mode);  // ctx option "qualities"
    int (*encode_qualities)(::ntc_ctx *ctx, ::ntc_qual_meta *metas, uint64_t meta_cap, uint8_t *payload,
                            uint64_t payload_cap, uint64_t *n_blocks, uint64_t *payload_bytes);
    int (*decode_set_qualities)(::ntc_ctx *ctx, const ::ntc_qual_meta *metas, uint64_t n_blocks, const uint8_t *payload,
                                uint64_t payload_bytes);
    int (*get_coder)(::ntc_ctx *ctx);  // ctx option "quality_coder" (0 pack, 1 rans), < 0: cannot be read
};
extern QHooks g_q_hooks;
// ... and for read names: with the table null, ntc_encode_file_ex2 / ntc_decode_file_ex2
// answer NTC_ERR_UNSUPPORTED to a name mode other than drop or to a name file.
struct NHooks {
    int (*set_mode)(::ntc_ctx *ctx, int mode);  // ctx option "names"
    int (*encode_names)(::ntc_ctx *ctx, ::ntc_name_meta *metas, uint64_t meta_cap, uint8_t *payload,
                        uint64_t payload_cap, uint64_t *n_blocks, uint64_t *payload_bytes);
    int (*decode_set_names)(::ntc_ctx *ctx, const ::ntc_name_meta *metas, uint64_t n_blocks, const uint8_t *payload,
                            uint64_t payload_bytes);
};
extern NHooks g_n_hooks;
// ... and for content digests: with the table null, ntc_encode_file_ex3 / ntc_decode_file_ex3
// answer NTC_ERR_UNSUPPORTED to d_mode 1, to a digest file and to out_fd -1.
struct DHooks {
    int (*set_mode)(::ntc_ctx *ctx, int on);  // ctx option "digests"
    int (*encode_digests)(::ntc_ctx *ctx, ::ntc_digest_meta *metas, uint64_t cap, uint64_t *n_blocks);
    int (*decode_set_digests)(::ntc_ctx *ctx, const ::ntc_digest_meta *metas, uint64_t n_blocks);
    int (*decode_digests)(::ntc_ctx *ctx, ::ntc_digest_meta *metas, uint64_t cap, uint64_t *n_blocks);
    int (*index_info)(::ntc_ctx *ctx, uint64_t *n_nodes, uint32_t *k);  // ntc_index_info
    int (*set_discard)(::ntc_ctx *ctx, int on);  // ctx option "discard_text"
};
extern DHooks g_d_hooks;
// ... and for paired-end reads: with the table null, ntc_encode_file_ex4 / ntc_decode_file_ex4
// answer NTC_ERR_UNSUPPORTED to pair_mode 1 and 2.
struct PHooks {
    int (*set_mode)(::ntc_ctx *ctx, int mode);  // ctx option "paired"
    int (*encode_paired)(::ntc_ctx *ctx, const uint8_t *fastq1, uint64_t bytes1, const uint8_t *fastq2, uint64_t bytes2,
                         uint64_t n_pairs, uint32_t block_reads, ::ntc_block_meta *meta, uint8_t **payload,
                         uint64_t *payload_bytes, uint64_t *n_bases, int64_t *bad_read);  // ntc_encode_pack_fastq_paired
    int (*pair_split)(::ntc_ctx *ctx, uint64_t *first_bytes);  // ntc_decode_pair_split
};
extern PHooks g_p_hooks;
// ... and for a range of reads: with the table null, ntc_decode_file_ex5 answers
// NTC_ERR_UNSUPPORTED to a range that does not start and end at block boundaries.
struct WHooks {
    int (*decode_set_window)(::ntc_ctx *ctx, uint64_t first, uint64_t count);  // ntc_decode_set_window
};
extern WHooks g_w_hooks;
// ... and for NTC_DEFLATE_GPU: with the table null, ntc_encode_file* answers NTC_ERR_UNSUPPORTED to it
struct ZHooks {
    int (*set_mode)(::ntc_ctx *ctx, int on);  // ctx option "gpu_deflate"
    int (*encode_members)(::ntc_ctx *ctx, uint64_t *member_off_len, uint64_t cap_blocks, uint64_t *n_blocks);
};
extern ZHooks g_z_hooks;
// ... and for BGZF output: with the table null, ntc_decode_file_ex7 answers NTC_ERR_UNSUPPORTED to
// out_format 1
struct BHooks {
    int (*set_mode)(::ntc_ctx *ctx, int on);  // ctx option "bgzf_text"
    int (*last_counts)(::ntc_ctx *ctx, ::ntc_bgzf_counts *counts);  // ntc_bgzf_last, the counts alone
};
extern BHooks g_b_hooks;
// ... and for `--inflate gpu`: an inflater lives on one device, with a stream, device buffers and a
// pinned staging buffer of its own (capi.cpp), and inflates a run of BGZF members from host memory
// into host memory (inflate.hip).  run: member i is m[i] of comp[0, comp_bytes) and goes to dst at
// its dst_off; the text is copied to dst only when every member is sound (*n_failed = 0).  With
// the table null, ntc_encode_file_ex6 answers NTC_ERR_UNSUPPORTED to inflate_engine 1.
struct Inflater;
struct IHooks {
    int (*create)(::ntc_ctx *ctx, Inflater **out);  // on ctx's device
    int (*run)(Inflater *inf, const uint8_t *comp, uint64_t comp_bytes, const ::ntc_inflate_member *m, uint64_t n,
               uint8_t *dst, uint64_t dst_bytes, uint64_t *n_failed);
    void (*destroy)(Inflater *inf);
};
extern IHooks g_i_hooks;
// what a reader did through its inflater
struct InflateCounts {
    uint64_t members = 0, bytes = 0;  // inflated on the device
    uint64_t runs = 0, fallback_runs = 0;  // calls, and those that delivered nothing (a member failed)
    double seconds = 0;  // inside the inflater
};
// fastx.cpp: ntc_fastx_open with an inflater (not owned) that a BGZF member reader uses from its
// first member on; true when fx is such a reader; add its counts to *out
int fastx_open_inflating(const char *path, Inflater *inf, ntc_fastx **out);
bool fastx_is_bgzf(ntc_fastx *fx);
void fastx_inflate_counts(ntc_fastx *fx, InflateCounts *out);
// the 32-byte header in front of stream s's gzip member of member_bytes bytes (block_codec.cpp)
void stream_header(uint8_t out[32], const ::ntc_block_meta &meta, int s, uint64_t member_bytes);
// libdeflate.so.0 loads: what `--deflate auto` asks
bool libdeflate_loaded();
struct PgzReader;
PgzReader *pgz_open(const char *path, int threads);
int pgz_read(PgzReader *r, char *dst, size_t cap, size_t *got);
void pgz_close(PgzReader *r);
}  // namespace ntc

struct ntc_index_host {
    ntc::HostIndex ix;
};
