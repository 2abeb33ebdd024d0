// ntcomp -- the command-line driver as a native binary: `ntcomp build | encode | decode`
// with the reference's flags (src/cli.rs:27-93) and stderr messages (src/main.rs:91-211),
// the hot path on the GPU through libntcomp_gpu.so's C ABI (include/*.h).  The Python CLI
// (`python -m ntcomp_amd`) is the same program; this one starts without an interpreter
// (the reference's binary is compiled code too), which is what a process-level timing sees.
//
//   ntcomp build -o P [-k 31] [-p 8] [-d] [-t 1] [-m 4] [--temp-dir D] [--verbose]
//                [-l LIST] [--builder auto|host|gpu] [--device N] [--index-format own|sbwt-rs] FILES...
//   ntcomp encode -i P [--gpus N | --devices 0,0,..] [--threads T] [--blocks-per-batch B]
//                 [--deflate auto|zlib|libdeflate|adaptive|gpu] [--host-parse] [--stats]
//                 [--non-acgt error|mask|keep] [--exceptions PATH]
//                 [--qualities drop|keep|bin8] [--quality-file PATH] [--quality-coder pack|rans]
//                 [--quality-smooth [M]] [--quality-smooth-to C]
//                 [--names drop|keep|id] [--name-file PATH] [--digest-file PATH]
//                 [--mate-file R2 | --interleaved] [--mate-check ids|off] FILE > encoded.dat
//                 (paired-end reads: FILE holds the mate-1 records and R2 the mate-2 records, or FILE
//                 is interleaved; the archive alternates the mates, whose ids are checked on the GPU)
//   ntcomp decode -i P [--gpus N | --devices ..] [--threads T] [--blocks-per-batch B] [--stats]
//                 [--exceptions PATH] [--quality-file PATH] [--name-file PATH] [--digest-file PATH]
//                 [--mate-out R2.out] [--bgzf] FILE > out.fasta
//                 (FASTQ with --quality-file, the reads' own names with --name-file; checked block by
//                 block against the --digest-file; with --mate-out the archive holds pairs: the mate-1
//                 records go to stdout, the mate-2 records to R2.out; --bgzf: the text as BGZF, compressed
//                 on the GPU, both outputs under --mate-out)
//   ntcomp verify -i P --digest-file PATH [--exceptions PATH] [--quality-file PATH] [--name-file PATH]
//                 FILE        (decode without the text: one line on stdout, status 0 iff every block matched)
#include <dlfcn.h>
#include <fcntl.h>
#include <unistd.h>

#include <chrono>
#include <ctime>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <thread>
#include <vector>

#include "../../include/ntcomp_codec.h"
#include "../../include/ntcomp_gpu.h"
#include "../../include/ntcomp_host.h"
#include "../../include/ntcomp_pipeline.h"

namespace {

using Clock = std::chrono::steady_clock;
constexpr const char *kVersion = "0.1.0";  // the reference's Cargo.toml version
double since(Clock::time_point t) { return std::chrono::duration<double>(Clock::now() - t).count(); }

[[noreturn]] void die(const std::string &msg) {
    std::fprintf(stderr, "ntcomp: %s\n", msg.c_str());
    std::exit(1);
}
void info(const char *msg) { std::fprintf(stderr, "%s\n", msg); }
// an argument error found after parsing: status 2, before anything is loaded or written
[[noreturn]] void bad_args(const std::string &msg) {
    std::fprintf(stderr, "ntcomp: %s\n", msg.c_str());
    std::exit(2);
}

struct Args {
    std::vector<std::string> pos;
    std::vector<std::pair<std::string, std::string>> kv;
    bool flag(const char *a, const char *b = nullptr) const {
        for (auto &p : kv)
            if (p.first == a || (b && p.first == b)) return true;
        return false;
    }
    std::string get(const char *a, const char *b, const std::string &def) const {
        std::string v = def;
        for (auto &p : kv)
            if (p.first == a || (b && p.first == b)) v = p.second;
        return v;
    }
};

// options taking a value, and switches; anything else starting with '-' is a usage error
// (clap rejects unknown arguments, src/cli.rs)
bool takes_value(const std::string &o) {
    static const char *v[] = {"-o", "--output-prefix", "-k", "-p", "--prefix-precalc", "-t", "--threads", "-m",
                              "--mem-gb", "--temp-dir", "-l", "--input-list", "--builder", "--device",
                              "--index-format", "-i", "--index", "--gpus", "--devices", "--blocks-per-batch",
                              "--deflate", "--inflate", "--contexts-per-gpu", "--non-acgt", "--exceptions",
                              "--qualities", "--quality-file", "--quality-coder", "--quality-smooth",
                              "--quality-smooth-to", "--names", "--name-file",
                              "--digest-file", "--mate-file", "--mate-check", "--mate-out", "--reads", "--shard"};
    for (const char *x : v)
        if (o == x) return true;
    return false;
}

bool is_switch(const std::string &o) {
    static const char *v[] = {"-d", "--dedup-batches", "--verbose", "--stats", "--host-parse", "--interleaved", "--blocks", "--bgzf"};
    for (const char *x : v)
        if (o == x) return true;
    return false;
}

void usage(FILE *f = stderr);

// all of s is decimal digits (at least one, at most 18: no overflow)
bool all_digits(const std::string &s) {
    if (s.empty() || s.size() > 18) return false;
    for (const char c : s)
        if (c < '0' || c > '9') return false;
    return true;
}

Args parse(int argc, char **argv, int from) {
    Args a;
    for (int i = from; i < argc; i++) {
        std::string s = argv[i];
        if (s.size() > 1 && s[0] == '-') {
            const size_t eq = s.find('=');
            if (s == "-h" || s == "--help") {  // clap: help on stdout, exit 0
                usage(stdout);
                std::exit(0);
            }
            if (s == "-V" || s == "--version") {
                std::printf("ntcomp %s\n", kVersion);
                std::exit(0);
            }
            if (s == "--quality-smooth" && !(i + 1 < argc && all_digits(argv[i + 1]))) {
                a.kv.push_back({s, "32"});  // the one flag whose value may be left out: the next argument only when a number
            } else if (s.size() > 2 && s[1] != '-' && takes_value(s.substr(0, 2))) {  // clap's attached short value: -t8, -k31
                a.kv.push_back({s.substr(0, 2), s.substr(2)});
            } else if (eq != std::string::npos && s.rfind("--", 0) == 0) {
                const std::string name = s.substr(0, eq);
                if (!takes_value(name)) die("unexpected argument '" + s + "'");
                a.kv.push_back({name, s.substr(eq + 1)});
            } else if (takes_value(s)) {
                if (i + 1 >= argc) die("option " + s + " needs a value");
                a.kv.push_back({s, argv[++i]});
            } else if (is_switch(s)) {
                a.kv.push_back({s, "1"});
            } else {
                die("unexpected argument '" + s + "'");
            }
        } else {
            a.pos.push_back(s);
        }
    }
    return a;
}

std::vector<int> devices_of(const Args &a) {
    std::vector<int> d;
    const std::string list = a.get("--devices", nullptr, "");
    if (!list.empty()) {
        size_t p = 0;
        while (p <= list.size()) {
            const size_t q = list.find(',', p);
            const std::string t = list.substr(p, q == std::string::npos ? std::string::npos : q - p);
            if (!t.empty()) d.push_back(std::atoi(t.c_str()));
            if (q == std::string::npos) break;
            p = q + 1;
        }
    } else {
        const int n = std::atoi(a.get("--gpus", nullptr, "1").c_str());
        for (int i = 0; i < n; i++) d.push_back(i);
    }
    if (d.empty()) die("no GPU given (--gpus / --devices)");
    return d;
}

// per_gpu contexts per listed device: the first uploads the index, the others on that device
// share it (ntc_index_share); batches alternate over all of them.  Encode: 2, so one call's
// H2D of FASTQ text overlaps the other's kernels (10 M x 150 bp, pipeline 6.2 -> 7.9 Gbases/s,
// profiles/round4/pipe_encode_gpu_parse_r04.jsonl); decode: 1 (2 measured no better).
constexpr int kEncodeContextsPerGpu = 2, kDecodeContextsPerGpu = 1;
// what encode / decode hand to main for the exit
std::vector<ntc_ctx *> g_ctxs;
ntc_index_host *g_ix = nullptr;
// decode_only: the upload builds what decode reads (the walk table), not the encoder's path
// cover, suffix table and SCAN words (ctx option decode_only)
std::vector<ntc_ctx *> open_gpus(const ntc_index_host *ix, const std::vector<int> &devs, int per_gpu,
                                 bool decode_only = false) {
    ntc_index_view v;
    if (ntc_index_view_of(ix, &v)) die("index view");
    // the HIP runtime starts (~0.1 s) while this thread derives the index's host tables
    std::vector<ntc_ctx *> ctxs(devs.size() * (size_t)(per_gpu > 0 ? per_gpu : 1), nullptr);
    std::vector<int> dev_of(ctxs.size());
    int create_rc = NTC_OK;
    std::thread creator([&] {
        for (size_t i = 0; i < ctxs.size(); i++) {
            dev_of[i] = devs[i / (size_t)(per_gpu > 0 ? per_gpu : 1)];
            const auto tc = Clock::now();
            if (ntc_ctx_create(dev_of[i], &ctxs[i])) {
                create_rc = NTC_ERR_HIP;
                dev_of[i] = -1;
                return;
            }
            // decode: start the device's DMA engines and load the unpacker's code object (HIP
            // loads one at its first launch) here beside the index preparation rather than on
            // the first batch's path: first batch decoded at 8 ms instead of 16-30, pipeline
            // 0.160 against 0.164 s (median of 4 on one box, profiles/round5/warm_ab/).  Encode
            // measured no better with the same (0.107 against 0.097 s), so it does not.
            if (std::getenv("NTC_INIT_TRACE"))
                std::fprintf(stderr, "[init] context %zu created in %.3f ms\n", i, 1e3 * since(tc));
            if (!decode_only || std::getenv("NTC_NO_WARM")) continue;
            (void)ntc_ctx_set_option(ctxs[i], "warm_dma", 4 << 20);
            ntc_block_meta m0{};
            uint8_t pay0[8] = {0};
            uint64_t ok = 0, nr = 0, nb = 0;
            (void)ntc_unpack_streams(ctxs[i], pay0, 8, &m0, 1, &ok, &nr, &nb);  // an empty block
        }
    });
    const auto ti = Clock::now();
    const bool itr = std::getenv("NTC_INIT_TRACE") != nullptr;  // start-up timeline on stderr
    ntc_index_prep *prep = nullptr;
    const int prep_rc = ntc_index_prepare(&v, &prep);
    if (itr) std::fprintf(stderr, "[init] %.3f ms index prepared\n", 1e3 * since(ti));
    creator.join();
    if (itr) std::fprintf(stderr, "[init] %.3f ms contexts created\n", 1e3 * since(ti));
    if (create_rc) {
        for (size_t i = 0; i < ctxs.size(); i++)
            if (dev_of[i] < 0) die("no usable GPU " + std::to_string(devs[i / (size_t)(per_gpu > 0 ? per_gpu : 1)]));
    }
    if (prep_rc) die("index: derived tables");
    std::vector<std::pair<int, ntc_ctx *>> first;
    for (size_t i = 0; i < ctxs.size(); i++) {
        ntc_ctx *c = ctxs[i], *src = nullptr;
        for (auto &f : first)
            if (f.first == dev_of[i]) src = f.second;
        if (src) {
            if (ntc_index_share(c, src)) die(std::string("index share: ") + ntc_last_error(c));
        } else {
            if (decode_only && ntc_ctx_set_option(c, "decode_only", 1)) die("ctx option decode_only");
            if (ntc_index_upload_prepared(c, prep)) die(std::string("index upload: ") + ntc_last_error(c));
            first.push_back({dev_of[i], c});
        }
    }
    ntc_index_prep_free(prep);
    if (itr) std::fprintf(stderr, "[init] %.3f ms index uploaded\n", 1e3 * since(ti));
    return ctxs;
}
int per_gpu_of(const Args &a, int def) {
    return std::atoi(a.get("--contexts-per-gpu", nullptr, std::to_string(def)).c_str());
}

bool libdeflate_present() {
    void *h = dlopen("libdeflate.so.0", RTLD_LAZY | RTLD_LOCAL);
    if (h) dlclose(h);
    return h != nullptr;
}

// --digest-file PATH as both commands take it: not empty, and no file the same call reads or writes
std::string digest_path_of(const Args &a, const char *cmd, const std::vector<std::string> &others) {
    if (!a.flag("--digest-file")) return "";
    const std::string d = a.get("--digest-file", nullptr, "");
    if (d.empty()) bad_args(std::string(cmd) + ": --digest-file needs a path");
    for (const std::string &o : others)
        if (!o.empty() && o == d) bad_args(std::string(cmd) + ": --digest-file names a file this call uses already: " + d);
    return d;
}
// "seq,sym" for a mask of NTC_DIGEST_* bits ("-" for none)
std::string component_names(uint32_t mask) {
    static const char *const names[4] = {"seq", "sym", "qual", "name"};
    std::string s;
    for (int c = 0; c < 4; c++)
        if (mask >> c & 1) s += (s.empty() ? "" : ",") + std::string(names[c]);
    return s.empty() ? "-" : s;
}

int cmd_encode(const Args &a) {
    const auto t0 = Clock::now();
    if (a.pos.size() != 1) die("encode: one query file");
    const std::string prefix = a.get("-i", "--index", "");
    // N and IUPAC symbols: error (default), mask, or keep with the exception runs in a side file
    const std::string nx_name = a.get("--non-acgt", nullptr, "error"), nx_path = a.get("--exceptions", nullptr, "");
    const int policy = nx_name == "error" ? NTC_NX_ERROR : nx_name == "mask" ? NTC_NX_MASK : nx_name == "keep" ? NTC_NX_KEEP : -1;
    if (policy < 0) bad_args("encode: --non-acgt: error, mask or keep");
    if (policy == NTC_NX_KEEP && nx_path.empty()) bad_args("encode: --non-acgt keep requires --exceptions PATH");
    if (policy != NTC_NX_KEEP && a.flag("--exceptions"))
        bad_args("encode: --exceptions is only written under --non-acgt keep");
    // quality scores: drop (default), keep, or bin8, with the packed sections in a side file
    const std::string q_name = a.get("--qualities", nullptr, "drop"), q_path = a.get("--quality-file", nullptr, "");
    const int q_mode = q_name == "drop" ? 0 : q_name == "keep" ? 1 : q_name == "bin8" ? 2 : -1;
    if (q_mode < 0) bad_args("encode: --qualities: drop, keep or bin8");
    if (q_mode > 0 && q_path.empty()) bad_args("encode: --qualities " + q_name + " requires --quality-file PATH");
    if (q_mode == 0 && a.flag("--quality-file"))
        bad_args("encode: --quality-file is only written under --qualities keep or bin8");
    // ... and their coder: pack (default; deflated on the host) or rans (coded on the GPU)
    const std::string qc_name = a.get("--quality-coder", nullptr, "pack");
    const int q_coder = qc_name == "pack" ? 0 : qc_name == "rans" ? 1 : -1;
    if (q_coder < 0) bad_args("encode: --quality-coder: pack or rans");
    if (q_mode == 0 && a.flag("--quality-coder")) bad_args("encode: --quality-coder needs --qualities keep or bin8");
    // ... smoothed inside long matches: --quality-smooth [M] (32 when left out), --quality-smooth-to C
    for (const char *f : {"--quality-smooth", "--quality-smooth-to"})
        if (q_mode == 0 && a.flag(f)) bad_args(std::string("encode: ") + f + " needs --qualities keep or bin8");
    const std::string qs_m = a.get("--quality-smooth", nullptr, "0"), qs_to = a.get("--quality-smooth-to", nullptr, "I");
    const bool qs_on = a.flag("--quality-smooth");
    if (qs_on && !(all_digits(qs_m) && qs_m.size() <= 8 && std::atol(qs_m.c_str()) >= 12 && std::atol(qs_m.c_str()) <= 16777215))
        bad_args("encode: --quality-smooth: M must be 12..16777215");
    if (qs_to.size() != 1 || qs_to[0] < '$' || qs_to[0] > '~')
        bad_args("encode: --quality-smooth-to: one printable byte in '$'..'~'");
    if (q_mode == 2 && a.flag("--quality-smooth-to") && qs_to[0] <= '*')
        bad_args("encode: --quality-smooth-to: under bin8 the byte must lie above '*', or its level is that of '#'");
    // read names: drop (default), keep, or id, with the front-coded sections in a side file
    const std::string n_name = a.get("--names", nullptr, "drop"), n_path = a.get("--name-file", nullptr, "");
    const int n_mode = n_name == "drop" ? 0 : n_name == "keep" ? 1 : n_name == "id" ? 2 : -1;
    if (n_mode < 0) bad_args("encode: --names: drop, keep or id");
    if (n_mode > 0 && n_path.empty()) bad_args("encode: --names " + n_name + " requires --name-file PATH");
    if (n_mode == 0 && a.flag("--name-file")) bad_args("encode: --name-file is only written under --names keep or id");
    // per-block content digests of everything this call encodes, for decode / verify --digest-file
    const std::string d_path = digest_path_of(a, "encode", {nx_path, q_path, n_path, a.pos[0]});
    // paired-end reads: the mate-2 file beside the input, or an interleaved input; the mates' ids are checked
    const std::string mate_path = a.get("--mate-file", nullptr, ""), check_name = a.get("--mate-check", nullptr, "ids");
    if (a.flag("--mate-file") && a.flag("--interleaved")) bad_args("encode: --mate-file and --interleaved exclude each other");
    if (a.flag("--mate-file") && mate_path.empty()) bad_args("encode: --mate-file needs a path");
    const bool pairs = a.flag("--mate-file") || a.flag("--interleaved");
    if (a.flag("--mate-check") && !pairs) bad_args("encode: --mate-check needs --mate-file or --interleaved");
    if (check_name != "ids" && check_name != "off") bad_args("encode: --mate-check: ids or off");
    if (pairs && a.flag("--host-parse")) bad_args("encode: pairs are woven and checked on the GPU: not with --host-parse");
    const int pair_mode = !pairs ? 0 : check_name == "ids" ? 1 : 2;
    // the engine of the block streams, settled before a GPU is opened
    std::string engine = a.get("--deflate", nullptr, "auto");
    if (engine != "auto" && engine != "zlib" && engine != "libdeflate" && engine != "adaptive" && engine != "gpu")
        bad_args("encode: --deflate: auto, zlib, libdeflate, adaptive or gpu");
    if (engine == "auto") engine = libdeflate_present() ? "adaptive" : "zlib";
    // ... and the engine that inflates a BGZF input: the first 18 bytes of every input decide
    const std::string inflate = a.get("--inflate", nullptr, "host");
    if (inflate != "host" && inflate != "gpu") bad_args("encode: --inflate: host or gpu");
    if (inflate == "gpu") {
        if (a.flag("--host-parse")) bad_args("encode: --inflate gpu feeds the GPU parser: not with --host-parse");
        for (const std::string &p : {a.pos[0], mate_path}) {
            if (p.empty()) continue;
            unsigned char h[18] = {0};
            FILE *f = std::fopen(p.c_str(), "rb");
            const size_t got = f ? std::fread(h, 1, 18, f) : 0;
            if (f) std::fclose(f);
            if (got != 18 || h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || !(h[3] & 4) || (h[10] | h[11] << 8) < 6 || h[12] != 'B' ||
                h[13] != 'C' || (h[16] | h[17] << 8) + 1 < 26)
                bad_args("encode: --inflate gpu: " + p + " does not start with a BGZF member");
        }
    }
    if (prefix.empty()) die("encode: -i/--index is required");
    info("Loading SBWT index...");
    ntc_index_host *ix = nullptr;
    if (ntc_index_load(prefix.c_str(), &ix)) die("cannot load index " + prefix);
    const double t_load = since(t0);
    auto ctxs = open_gpus(ix, devices_of(a), per_gpu_of(a, kEncodeContextsPerGpu));
    const double t_gpu = since(t0);
    info("Encoding fastX data...");
    ntc_pipeline_opts o{};
    o.threads = std::atoi(a.get("--threads", nullptr, "0").c_str());
    o.blocks_per_batch = std::atoi(a.get("--blocks-per-batch", nullptr, "4").c_str());
    o.deflate_engine = engine == "adaptive"     ? NTC_DEFLATE_ADAPTIVE
                       : engine == "libdeflate" ? NTC_DEFLATE_LIBDEFLATE
                       : engine == "gpu"        ? NTC_DEFLATE_GPU
                                                : NTC_DEFLATE_ZLIB;
    o.host_parse = a.flag("--host-parse") ? 1 : 0;
    ntc_pipeline_stats st{};
    ntc_nx_stats nx{};
    int nx_fd = -1;
    if (policy == NTC_NX_KEEP && (nx_fd = ::open(nx_path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644)) < 0)
        die("encode: cannot write " + nx_path);
    ntc_q_stats qs{};
    int q_fd = -1;
    if (q_mode > 0 && (q_fd = ::open(q_path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644)) < 0)
        die("encode: cannot write " + q_path);
    ntc_n_stats ns{};
    int n_fd = -1;
    if (n_mode > 0 && (n_fd = ::open(n_path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644)) < 0)
        die("encode: cannot write " + n_path);
    ntc_d_stats dst{};
    int d_fd = -1;
    if (!d_path.empty() && (d_fd = ::open(d_path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644)) < 0)
        die("encode: cannot write " + d_path);
    if (q_mode > 0)  // the pipeline takes the coder from its contexts
        for (ntc_ctx *c : ctxs)
            if (ntc_ctx_set_option(c, "quality_coder", q_coder)) die("encode: --quality-coder: the option was refused");
    if (q_mode > 0)  // ... and the smoothing
        for (ntc_ctx *c : ctxs)
            if (ntc_ctx_set_option(c, "quality_smooth", qs_on ? std::atol(qs_m.c_str()) : 0) ||
                ntc_ctx_set_option(c, "quality_smooth_to", qs_to[0]))
                die("encode: --quality-smooth: the option was refused");
    const ntc_file_opts fo{policy, nx_fd, q_mode, q_fd, nullptr, nullptr};
    const ntc_file_opts2 fo2{(uint32_t)sizeof(ntc_file_opts2), policy, nx_fd, q_mode, q_fd, nullptr, nullptr, n_mode, n_fd, nullptr};
    const ntc_file_opts3 fo3{(uint32_t)sizeof(ntc_file_opts3), policy, nx_fd, q_mode, q_fd, nullptr, nullptr, n_mode, n_fd,
                             nullptr, 1, d_fd, nullptr};
    const ntc_file_opts4 fo4{(uint32_t)sizeof(ntc_file_opts4), policy, nx_fd, q_mode, q_fd, nullptr, nullptr, n_mode, n_fd,
                             nullptr, d_fd >= 0 ? 1 : 0, d_fd, nullptr, pair_mode, mate_path.empty() ? nullptr : mate_path.c_str(), -1};
    ntc_p_stats pst{};
    ntc_i_stats ist{};
    const ntc_file_opts6 fo6{(uint32_t)sizeof(ntc_file_opts6), policy, nx_fd, q_mode, q_fd, nullptr, nullptr, n_mode, n_fd, nullptr,
                             d_fd >= 0 ? 1 : 0, d_fd, nullptr, pair_mode, mate_path.empty() ? nullptr : mate_path.c_str(), -1, 0, 0,
                             NTC_INFLATE_GPU, 0};
    std::fflush(stdout);
    const int rc = inflate == "gpu" ? ntc_encode_file_ex6(ctxs.data(), (int)ctxs.size(), a.pos[0].c_str(), 1, &fo6, &o, &st, &nx, &qs, &ns, &dst, &pst, &ist)
                   : pair_mode ? ntc_encode_file_ex4(ctxs.data(), (int)ctxs.size(), a.pos[0].c_str(), 1, &fo4, &o, &st, &nx, &qs, &ns, &dst, &pst)
                   : d_fd >= 0 ? ntc_encode_file_ex3(ctxs.data(), (int)ctxs.size(), a.pos[0].c_str(), 1, &fo3, &o, &st, &nx, &qs, &ns, &dst)
                   : n_mode > 0 ? ntc_encode_file_ex2(ctxs.data(), (int)ctxs.size(), a.pos[0].c_str(), 1, &fo2, &o, &st, &nx, &qs, &ns)
                   : q_mode > 0 ? ntc_encode_file_ex(ctxs.data(), (int)ctxs.size(), a.pos[0].c_str(), 1, &fo, &o, &st, &nx, &qs)
                   : policy == NTC_NX_ERROR
                       ? ntc_encode_file(ctxs.data(), (int)ctxs.size(), a.pos[0].c_str(), 1, &o, &st)
                       : ntc_encode_file_nx(ctxs.data(), (int)ctxs.size(), a.pos[0].c_str(), 1, policy, nx_fd, &o, &st, &nx);
    if (nx_fd >= 0 && ::close(nx_fd) != 0 && rc == NTC_OK) die("encode: cannot write " + nx_path);
    if (q_fd >= 0 && ::close(q_fd) != 0 && rc == NTC_OK) die("encode: cannot write " + q_path);
    if (n_fd >= 0 && ::close(n_fd) != 0 && rc == NTC_OK) die("encode: cannot write " + n_path);
    if (d_fd >= 0 && ::close(d_fd) != 0 && rc == NTC_OK) die("encode: cannot write " + d_path);
    char qjson[2048] = "";  // the quality and name files' figures, when they were written
    if (q_mode > 0)
        std::snprintf(qjson, 320, "\"qualities\": \"%s\", \"quality_coder\": \"%s\", \"q_sections\": %llu, "
                                  "\"q_quals\": %llu, \"q_packed_bytes\": %llu, \"q_deflated_bytes\": %llu, ",
                      q_name.c_str(), qc_name.c_str(), (unsigned long long)qs.sections, (unsigned long long)qs.quals,
                      (unsigned long long)qs.packed_bytes, (unsigned long long)qs.deflated_bytes);
    if (qs_on) {
        unsigned long long smoothed = 0;
        for (ntc_ctx *c : ctxs) {
            int64_t v = 0;
            if (ntc_ctx_get_option(c, "quality_smoothed_total", &v) == NTC_OK) smoothed += (unsigned long long)v;
        }
        const std::string to_json = qs_to == "\\" ? "\\\\" : qs_to;  // (the one byte of the range that JSON escapes)
        std::snprintf(qjson + std::strlen(qjson), 160, "\"quality_smooth\": %ld, \"quality_smooth_to\": \"%s\", "
                                                       "\"q_smoothed\": %llu, ",
                      std::atol(qs_m.c_str()), to_json.c_str(), smoothed);
    }
    if (n_mode > 0)
        std::snprintf(qjson + std::strlen(qjson), 320, "\"names\": \"%s\", \"n_sections\": %llu, \"n_names\": %llu, "
                                                       "\"n_name_bytes\": %llu, \"n_payload_bytes\": %llu, "
                                                       "\"n_deflated_bytes\": %llu, ",
                      n_name.c_str(), (unsigned long long)ns.sections, (unsigned long long)ns.names,
                      (unsigned long long)ns.name_bytes, (unsigned long long)ns.payload_bytes,
                      (unsigned long long)ns.deflated_bytes);
    if (d_fd >= 0)
        std::snprintf(qjson + std::strlen(qjson), 250, "\"d_sections\": %llu, \"d_blocks_seq\": %llu, \"d_blocks_sym\": %llu, "
                                                       "\"d_blocks_qual\": %llu, \"d_blocks_name\": %llu, ",
                      (unsigned long long)dst.sections, (unsigned long long)dst.blocks_seq, (unsigned long long)dst.blocks_sym,
                      (unsigned long long)dst.blocks_qual, (unsigned long long)dst.blocks_name);
    if (pair_mode)
        std::snprintf(qjson + std::strlen(qjson), 250, "\"pairs\": %llu, \"mate_check\": \"%s\", \"mate1_bytes\": %llu, "
                                                       "\"mate2_bytes\": %llu, ",
                      (unsigned long long)pst.pairs, check_name.c_str(), (unsigned long long)pst.bytes1,
                      (unsigned long long)pst.bytes2);
    std::snprintf(qjson + std::strlen(qjson), 250, "\"inflate\": \"%s\", \"inflate_members\": %llu, \"inflate_bytes\": %llu, "
                                                   "\"inflate_runs\": %llu, \"inflate_fallback_runs\": %llu, \"inflate_s\": %.3f, ",
                  inflate.c_str(), (unsigned long long)ist.members, (unsigned long long)ist.bytes, (unsigned long long)ist.runs,
                  (unsigned long long)ist.fallback_runs, ist.seconds);
    g_ctxs = ctxs;  // main frees the contexts and the host index before leaving
    g_ix = ix;
    if (rc) {
        std::string m = std::string("encode: ") + st.error;
        if (st.bad_read >= 0) m += " (read " + std::to_string(st.bad_read + 1) + ")";
        die(m);
    }
    if (st.dropped_blocks)
        std::fprintf(stderr, "warning: %llu block(s) dropped (no long or no short records; main.rs:170 ignores "
                             "write_block_to's error, SURVEY App. B.3)\n",
                     (unsigned long long)st.dropped_blocks);
    if (a.flag("--stats"))
        std::fprintf(stderr,
                     "{\"stats\": {\"index_load\": %.3f, \"gpu_init_upload\": %.3f, \"parse\": %.3f, \"gpu\": %.3f, "
                     "\"deflate\": %.3f, \"write\": %.3f}, \"command\": \"encode\", \"native\": true, \"gpus\": %zu, "
                     "\"threads\": %d, \"reads\": %llu, \"blocks\": %llu, \"dropped_blocks\": %llu, "
                     "\"pipeline_wall_s\": %.3f, \"deflate\": \"%s\", \"gpu_parsed_batches\": %d, \"non_acgt\": \"%s\", "
                     "\"nx_runs\": %llu, \"nx_bases\": %llu, \"nx_reads\": %llu, \"nx_runs_in_dropped_blocks\": %llu, "
                     "%s\"process_s\": %.3f}\n",
                     t_load, t_gpu - t_load, st.parse_s, st.gpu_s, st.deflate_s, st.write_s, ctxs.size(), st.threads,
                     (unsigned long long)st.reads, (unsigned long long)st.blocks,
                     (unsigned long long)st.dropped_blocks, st.wall_s, engine.c_str(), st.gpu_parsed, nx_name.c_str(),
                     (unsigned long long)nx.runs, (unsigned long long)nx.bases, (unsigned long long)nx.reads,
                     (unsigned long long)nx.runs_in_dropped_blocks, qjson, since(t0));
    return 0;
}

// the pipeline's stream decode on the host pool (NTC_HOST_UNPACK, pipeline.cpp) -- for --stats
bool host_unpack_on() {
    const char *h = std::getenv("NTC_HOST_UNPACK");
    return h && std::atoi(h) > 0;
}

// --reads A-B, 1-based and inclusive as decode prints seq.N; also A, A- and -B.  *b = 0: to the
// last read.  false: malformed.
bool parse_reads(const std::string &spec, uint64_t *a, uint64_t *b) {
    const size_t dash = spec.find('-');
    const std::string lo = spec.substr(0, dash), hi = dash == std::string::npos ? lo : spec.substr(dash + 1);
    if (lo.empty() && hi.empty()) return false;
    if ((!lo.empty() && !all_digits(lo)) || (!hi.empty() && !all_digits(hi))) return false;
    *a = lo.empty() ? 1 : std::strtoull(lo.c_str(), nullptr, 10);
    *b = hi.empty() ? 0 : std::strtoull(hi.c_str(), nullptr, 10);
    return *a >= 1 && (hi.empty() || *b >= *a);
}

// --shard I/N with 1 <= I <= N
bool parse_shard(const std::string &spec, uint64_t *i, uint64_t *n) {
    const size_t slash = spec.find('/');
    if (slash == std::string::npos || !all_digits(spec.substr(0, slash)) || !all_digits(spec.substr(slash + 1))) return false;
    *i = std::strtoull(spec.c_str(), nullptr, 10);
    *n = std::strtoull(spec.c_str() + slash + 1, nullptr, 10);
    return *i >= 1 && *i <= *n;
}

// what --reads / --shard ask, checked from the arguments alone, then placed against the block
// headers (host only): reads [first, first + count) from 0
struct RangeAsk {
    bool reads = false, shard = false;
    uint64_t a = 0, b = 0, i = 0, n = 0;
    std::string spec;
};
RangeAsk range_args(const Args &a, const char *cmd) {
    RangeAsk r;
    if (a.flag("--reads") && a.flag("--shard")) bad_args(std::string(cmd) + ": --reads and --shard exclude each other");
    if (a.flag("--reads")) {
        r.reads = true;
        r.spec = a.get("--reads", nullptr, "");
        if (!parse_reads(r.spec, &r.a, &r.b))
            bad_args(std::string(cmd) + ": --reads " + r.spec + ": want A-B, A, A- or -B (1-based, inclusive, 1 <= A <= B)");
        if (a.flag("--mate-out") && (r.a % 2 == 0 || (r.b && r.b % 2 == 1)))
            bad_args(std::string(cmd) + ": --reads " + r.spec + " with --mate-out: whole pairs start at an odd read and end at an even one");
    }
    if (a.flag("--shard")) {
        r.shard = true;
        r.spec = a.get("--shard", nullptr, "");
        if (!parse_shard(r.spec, &r.i, &r.n)) bad_args(std::string(cmd) + ": --shard " + r.spec + ": want I/N with 1 <= I <= N");
    }
    return r;
}
// false: an empty slice
bool place_range(const RangeAsk &r, const Args &a, const char *cmd, uint64_t *first, uint64_t *count) {
    ntc_archive_block *blocks = nullptr;
    uint64_t nb = 0, total = 0;
    if (ntc_archive_info(a.pos[0].c_str(), &blocks, &nb, &total, nullptr, nullptr)) die(std::string(cmd) + ": cannot read " + a.pos[0]);
    if (r.reads) {
        ntc_buffer_free(blocks);
        const uint64_t b = r.b ? r.b : total;
        if (r.a > total || b > total)
            bad_args(std::string(cmd) + ": --reads " + r.spec + ": the archive holds " + std::to_string(total) + " reads");
        if (a.flag("--mate-out") && b % 2) bad_args(std::string(cmd) + ": --reads " + r.spec + " with --mate-out: the range ends inside a pair");
        *first = r.a - 1;
        *count = b - r.a + 1;
        return true;
    }
    const uint64_t lo = (r.i - 1) * nb / r.n, hi = r.i * nb / r.n;
    *first = *count = 0;
    for (uint64_t k = 0; k < hi; k++) (k < lo ? *first : *count) += blocks[k].reads;
    ntc_buffer_free(blocks);
    if (*count && a.flag("--mate-out") && *first % 2)
        bad_args(std::string(cmd) + ": --shard " + r.spec + " with --mate-out: the slice starts inside a pair");
    return *count != 0;
}

// `ntcomp info encoded.dat [--blocks]`: what the archive holds, from its block headers alone;
// no index, no GPU.  Status 1 when a block's headers are damaged.
int cmd_info(const Args &a) {
    if (a.pos.size() != 1) die("info: one input file");
    ntc_archive_block *blocks = nullptr;
    uint64_t nb = 0, reads = 0, recs = 0, tail = 0, bytes = 0, bad = 0;
    if (ntc_archive_info(a.pos[0].c_str(), &blocks, &nb, &reads, &recs, &tail)) die("info: cannot read " + a.pos[0]);
    for (uint64_t i = 0; i < nb; i++) bytes += blocks[i].bytes, bad += blocks[i].bad;
    std::printf("blocks %llu reads %llu records %llu bytes %llu trailing_bytes %llu", (unsigned long long)nb,
                (unsigned long long)reads, (unsigned long long)recs, (unsigned long long)bytes, (unsigned long long)tail);
    if (bad) std::printf(" damaged_blocks %llu", (unsigned long long)bad);
    std::printf("\n");
    uint64_t first = 1;
    for (uint64_t i = 0; a.flag("--blocks") && i < nb; i++) {
        std::printf("block %llu offset %llu bytes %llu reads %llu records %llu ", (unsigned long long)i,
                    (unsigned long long)blocks[i].offset, (unsigned long long)blocks[i].bytes,
                    (unsigned long long)blocks[i].reads, (unsigned long long)blocks[i].records);
        if (blocks[i].bad) std::printf("damaged\n");
        else std::printf("first_read %llu\n", (unsigned long long)first);
        first += blocks[i].reads;
    }
    ntc_buffer_free(blocks);
    std::fflush(stdout);
    return bad ? 1 : 0;
}

// verify: decode with out_fd -1 -- nothing is copied off the device or written; one line on stdout
int cmd_decode(const Args &a, bool verify = false) {
    const auto t0 = Clock::now();
    const char *cmd = verify ? "verify" : "decode";
    if (a.pos.size() != 1) die(std::string(cmd) + ": one input file");
    const std::string prefix = a.get("-i", "--index", "");
    const std::string d_path = digest_path_of(a, cmd, {a.get("--exceptions", nullptr, ""), a.get("--quality-file", nullptr, ""),
                                                       a.get("--name-file", nullptr, ""), a.pos[0]});
    if (verify && d_path.empty()) bad_args("verify: --digest-file PATH is required");
    // a paired archive: the mate-1 records to stdout, the mate-2 records to --mate-out
    const std::string mate_out = a.get("--mate-out", nullptr, "");
    if (verify && a.flag("--mate-out")) bad_args("verify: writes no text: not with --mate-out");
    if (a.flag("--mate-out") && mate_out.empty()) bad_args("decode: --mate-out needs a path");
    // the text as BGZF members, compressed on the GPU that formatted it
    const bool bgzf = a.flag("--bgzf");
    if (verify && bgzf) bad_args("verify: writes no text: not with --bgzf");
    const RangeAsk ask = range_args(a, cmd);
    if (prefix.empty()) die(std::string(cmd) + ": -i/--index is required");
    const bool ranged = ask.reads || ask.shard;
    uint64_t r_first = 0, r_count = 0;
    if (ranged && !place_range(ask, a, cmd, &r_first, &r_count)) {  // an empty slice: nothing to write
        if (verify) std::printf("verify: OK: 0 blocks of the archive's, 0 reads (--shard %s is empty)\n", ask.spec.c_str());
        if (bgzf) {  // an empty BGZF file is its EOF member
            const int fde = mate_out.empty() ? -1 : ::open(mate_out.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
            if (::write(1, NTC_BGZF_EOF, NTC_BGZF_EOF_BYTES) != NTC_BGZF_EOF_BYTES ||
                (!mate_out.empty() && (fde < 0 || ::write(fde, NTC_BGZF_EOF, NTC_BGZF_EOF_BYTES) != NTC_BGZF_EOF_BYTES || ::close(fde) != 0)))
                die("decode: cannot write the output");
        }
        return 0;
    }
    ntc_index_host *ix = nullptr;
    if (ntc_index_load(prefix.c_str(), &ix)) die("cannot load index " + prefix);
    const double t_load = since(t0);
    auto ctxs = open_gpus(ix, devices_of(a), per_gpu_of(a, kDecodeContextsPerGpu), true);
    const double t_gpu = since(t0);
    info(verify ? "Verifying encoded data..." : "Decoding encoded data...");
    ntc_pipeline_opts o{};
    o.threads = std::atoi(a.get("--threads", nullptr, "0").c_str());
    o.blocks_per_batch = std::atoi(a.get("--blocks-per-batch", nullptr, "2").c_str());
    ntc_pipeline_stats st{};
    const std::string nx_path = a.get("--exceptions", nullptr, "");  // the side file of encode --non-acgt keep
    const std::string q_path = a.get("--quality-file", nullptr, "");  // ... of encode --qualities keep: FASTQ out
    const ntc_file_opts fo{0, -1, 0, -1, nx_path.empty() ? nullptr : nx_path.c_str(), q_path.c_str()};
    const std::string n_path = a.get("--name-file", nullptr, "");  // ... of encode --names keep: the reads' names
    const ntc_file_opts2 fo2{(uint32_t)sizeof(ntc_file_opts2), 0, -1, 0, -1, fo.nx_path,
                             q_path.empty() ? nullptr : q_path.c_str(), 0, -1, n_path.c_str()};
    const ntc_file_opts3 fo3{(uint32_t)sizeof(ntc_file_opts3), 0, -1, 0, -1, fo.nx_path, fo2.q_path, 0, -1,
                             n_path.empty() ? nullptr : n_path.c_str(), 0, -1, d_path.c_str()};
    ntc_d_stats dst{};
    int fd2 = -1;
    if (!mate_out.empty() && (fd2 = ::open(mate_out.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644)) < 0)
        die("decode: cannot write " + mate_out);
    const ntc_file_opts4 fo4{(uint32_t)sizeof(ntc_file_opts4), 0, -1, 0, -1, fo.nx_path, fo2.q_path, 0, -1, fo3.n_path, 0, -1,
                             d_path.empty() ? nullptr : d_path.c_str(), 2, nullptr, fd2};
    ntc_p_stats pst{};
    const ntc_file_opts5 fo5{(uint32_t)sizeof(ntc_file_opts5), 0, -1, 0, -1, fo.nx_path, fo2.q_path, 0, -1, fo3.n_path, 0, -1,
                             fo4.d_path, fd2 >= 0 ? 2 : 0, nullptr, fd2, r_first, r_count};
    ntc_r_stats rst{};
    const ntc_file_opts7 fo7{(uint32_t)sizeof(ntc_file_opts7), 0, -1, 0, -1, fo.nx_path, fo2.q_path, 0, -1, fo3.n_path, 0, -1,
                             fo4.d_path, fd2 >= 0 ? 2 : 0, nullptr, fd2, r_first, r_count, 0, 0, NTC_OUT_BGZF, 0};
    ntc_z_stats zst{};
    std::fflush(stdout);
    const int rc = bgzf ? ntc_decode_file_ex7(ctxs.data(), (int)ctxs.size(), a.pos[0].c_str(), 1, &fo7, &o, &st, &dst, &pst, &rst, &zst)
                   : ranged ? ntc_decode_file_ex5(ctxs.data(), (int)ctxs.size(), a.pos[0].c_str(), verify ? -1 : 1, &fo5, &o, &st, &dst, &pst, &rst)
                   : fd2 >= 0 ? ntc_decode_file_ex4(ctxs.data(), (int)ctxs.size(), a.pos[0].c_str(), 1, &fo4, &o, &st, &dst, &pst)
                   : !d_path.empty() ? ntc_decode_file_ex3(ctxs.data(), (int)ctxs.size(), a.pos[0].c_str(), verify ? -1 : 1, &fo3, &o, &st, &dst)
                   : !n_path.empty() ? ntc_decode_file_ex2(ctxs.data(), (int)ctxs.size(), a.pos[0].c_str(), 1, &fo2, &o, &st)
                   : !q_path.empty() ? ntc_decode_file_ex(ctxs.data(), (int)ctxs.size(), a.pos[0].c_str(), 1, &fo, &o, &st)
                   : nx_path.empty()
                       ? ntc_decode_file(ctxs.data(), (int)ctxs.size(), a.pos[0].c_str(), 1, &o, &st)
                       : ntc_decode_file_nx(ctxs.data(), (int)ctxs.size(), a.pos[0].c_str(), nx_path.c_str(), 1, &o, &st);
    if (fd2 >= 0 && ::close(fd2) != 0 && rc == NTC_OK) die("decode: cannot write " + mate_out);
    g_ctxs = ctxs;  // main frees the contexts and the host index before leaving
    g_ix = ix;
    if (rc) {
        std::string m = std::string(cmd) + ": " + st.error;
        if (rc == NTC_ERR_DIGEST && st.bad_read >= 0) m += " (read " + std::to_string(st.bad_read + 1) + ")";
        die(m);
    }
    const std::string of = ranged ? " of " + std::to_string(rst.blocks_total) : "";
    if (verify)
        std::printf("verify: OK: %llu%s blocks, %llu reads, checked %s, not checkable %s\n", (unsigned long long)dst.sections,
                    of.c_str(), (unsigned long long)st.reads,
                    component_names((dst.blocks_seq ? 1u : 0) | (dst.blocks_sym ? 2u : 0) | (dst.blocks_qual ? 4u : 0) |
                                    (dst.blocks_name ? 8u : 0)).c_str(),
                    component_names(dst.not_checkable).c_str());
    char djson[1400] = "";
    if (fd2 >= 0)
        std::snprintf(djson, 240, "\"pairs\": %llu, \"mate1_bytes\": %llu, \"mate2_bytes\": %llu, ",
                      (unsigned long long)pst.pairs, (unsigned long long)pst.bytes1, (unsigned long long)pst.bytes2);
    if (!d_path.empty())
        std::snprintf(djson + std::strlen(djson), 320, "\"d_sections\": %llu, \"d_blocks_seq\": %llu, \"d_blocks_sym\": %llu, "
                                            "\"d_blocks_qual\": %llu, \"d_blocks_name\": %llu, \"d_not_checkable\": \"%s\", ",
                      (unsigned long long)dst.sections, (unsigned long long)dst.blocks_seq, (unsigned long long)dst.blocks_sym,
                      (unsigned long long)dst.blocks_qual, (unsigned long long)dst.blocks_name,
                      component_names(dst.not_checkable).c_str());
    if (ranged)
        std::snprintf(djson + std::strlen(djson), 400, "\"r_blocks_total\": %llu, \"r_reads_total\": %llu, \"r_first_block\": %llu, "
                                            "\"r_blocks_read\": %llu, \"r_reads_written\": %llu, \"r_head_skipped\": %llu, "
                                            "\"r_tail_skipped\": %llu, ",
                      (unsigned long long)rst.blocks_total, (unsigned long long)rst.reads_total, (unsigned long long)rst.first_block,
                      (unsigned long long)rst.blocks_read, (unsigned long long)rst.reads_written,
                      (unsigned long long)rst.head_skipped, (unsigned long long)rst.tail_skipped);
    if (!verify)
        std::snprintf(djson + std::strlen(djson), 400, "\"bgzf\": %s, \"bgzf_members\": %llu, \"bgzf_text_bytes\": %llu, "
                                            "\"bgzf_bytes\": %llu, \"bgzf_chunks_stored\": %llu, \"bgzf_chunks_huffman\": %llu, "
                                            "\"bgzf_chunks_matches\": %llu, \"bgzf_s\": %.3f, ",
                      bgzf ? "true" : "false", (unsigned long long)zst.members, (unsigned long long)zst.text_bytes,
                      (unsigned long long)zst.bytes, (unsigned long long)zst.chunks_stored, (unsigned long long)zst.chunks_huffman,
                      (unsigned long long)zst.chunks_matches, zst.seconds);
    if (st.dropped_blocks)  // the reference's `while let Ok(..) = decode_block` just ends here (main.rs:202)
        std::fprintf(stderr, "warning: %s; %llu block(s) not decoded\n", st.error,
                     (unsigned long long)st.dropped_blocks);
    if (a.flag("--stats"))
        std::fprintf(stderr,
                     "{\"stats\": {\"index_load\": %.3f, \"gpu_init_upload\": %.3f, \"unzip\": %.3f, \"gpu\": %.3f, "
                     "\"write\": %.3f, \"alloc\": %.3f}, \"timeline\": {\"first_write\": %.3f, \"unzip_done\": %.3f, "
                     "\"gpu_done\": %.3f}, \"command\": \"%s\", \"native\": true, \"gpus\": %zu, \"threads\": %d, "
                     "\"reads\": %llu, \"blocks\": %llu, \"pipeline_wall_s\": %.3f, \"gpu_unpack\": %s, "
                     "%s\"process_s\": %.3f}\n",
                     t_load, t_gpu - t_load, st.parse_s, st.gpu_s, st.write_s, st.alloc_s, st.first_batch_s,
                     st.reader_done_s, st.gpu_done_s, cmd, ctxs.size(), st.threads, (unsigned long long)st.reads,
                     (unsigned long long)st.blocks, st.wall_s, host_unpack_on() ? "false" : "true", djson, since(t0));
    return 0;
}

// --input-list: one path, or tab-separated name and path, per line (main.rs:64-89)
std::vector<std::string> read_list(const std::string &path) {
    std::vector<std::string> out;
    std::ifstream f(path);
    if (!f) die("cannot read " + path);
    std::string line;
    while (std::getline(f, line)) {
        if (line.empty()) continue;
        const size_t t = line.find('\t');
        out.push_back(t == std::string::npos ? line : line.substr(t + 1));
    }
    return out;
}

int cmd_build(const Args &a) {
    std::vector<std::string> files = a.pos;
    const std::string list = a.get("-l", "--input-list", "");
    if (!list.empty())
        for (auto &p : read_list(list)) files.push_back(p);
    if (files.empty()) die("build: no input files");
    const std::string prefix = a.get("-o", "--output-prefix", "");
    if (prefix.empty()) die("build: -o/--output-prefix is required");
    const uint32_t k = (uint32_t)std::atoi(a.get("-k", nullptr, "31").c_str());
    const uint32_t pre = (uint32_t)std::atoi(a.get("-p", "--prefix-precalc", "8").c_str());
    const int threads = std::atoi(a.get("-t", "--threads", "1").c_str());
    const double mem_gb = std::atof(a.get("-m", "--mem-gb", "4").c_str());
    const bool mem_given = a.flag("-m", "--mem-gb");
    const std::string temp = a.get("--temp-dir", nullptr, "");
    const std::string builder = a.get("--builder", nullptr, "auto");
    const std::string layout = a.get("--index-format", nullptr, "sbwt-rs");
    const int device = std::atoi(a.get("--device", nullptr, "0").c_str());
    const bool verbose = a.flag("--verbose");
    std::fprintf(stderr, "Building SBWT index from %zu files...\n", files.size());
    // every sequence of every file, back to back (main.rs:37-62: read_fastx_file per file)
    std::vector<uint8_t> seq;
    std::vector<uint64_t> offs{0};
    for (const auto &path : files) {
        ntc_fastx *fx = nullptr;
        if (ntc_fastx_open(path.c_str(), &fx)) die("cannot read " + path);
        for (;;) {
            const uint8_t *b;
            const uint64_t *o;
            uint64_t n = 0;
            const int rc = ntc_fastx_next_batch(fx, 1u << 16, 1ull << 28, &b, &o, &n);
            if (rc) die("malformed or unreadable input: " + path);
            if (!n) break;
            seq.insert(seq.end(), b + o[0], b + o[n]);
            const uint64_t base = offs.back() - o[0];
            for (uint64_t r = 1; r <= n; r++) offs.push_back(base + o[r]);
        }
        ntc_fastx_close(fx);
    }
    ntc_index_host *ix = nullptr;
    ntc_ctx *ctx = nullptr;
    if (builder != "host" && ntc_ctx_create(device, &ctx) != NTC_OK) {
        if (builder == "gpu") die("--builder gpu: no usable GPU " + std::to_string(device));
        ctx = nullptr;
    }
    if (ctx) {
        // kbo's BuildOpts { mem_gb, temp_dir } (main.rs:111-134; cli.rs:55-60: --temp-dir builds
        // "on temporary disk space instead of in-memory", -m is the memory for that).  -m given:
        // the device memory of a pass; else 85 % of the free HBM.  --temp-dir given: sorted
        // partitions past -m GB of host memory go to files there; else nothing spills.
        ntc_build_opts o{};
        const uint64_t mem = (uint64_t)(mem_gb * (double)(1ull << 30));
        o.device_budget_bytes = mem_given ? mem : 0;
        o.host_budget_bytes = temp.empty() ? 0 : mem;
        o.temp_dir = temp.empty() ? nullptr : temp.c_str();
        ntc_build_stats st{};
        const int rc = ntc_build_index_device_ex(ctx, seq.data(), offs.data(), offs.size() - 1, k, 1, &o, &st, &ix);
        if (rc) die(std::string("build: ") + ntc_last_error(ctx));
        ntc_ctx_destroy(ctx);
        if (verbose)
            std::fprintf(stderr,
                         "build: %llu occurrences, %llu k-mers, %llu nodes, %u + %u passes, %.3f s (GPU, budget %llu "
                         "B, peak %llu B, spilled %llu B)\n",
                         (unsigned long long)st.occurrences, (unsigned long long)st.kmers,
                         (unsigned long long)st.nodes, st.kmer_partitions, st.node_partitions, st.seconds,
                         (unsigned long long)st.device_budget_bytes, (unsigned long long)st.peak_device_bytes,
                         (unsigned long long)st.spilled_bytes);
    } else {
        if (ntc_build_index(seq.data(), offs.data(), offs.size() - 1, k, 1, threads, &ix)) die("build failed");
    }
    const int lay = layout == "sbwt-rs" ? NTC_INDEX_SBWT_RS : NTC_INDEX_OWN;
    if (lay == NTC_INDEX_SBWT_RS && pre) ntc_index_set_prefix_precalc(ix, pre < k ? (pre < 12 ? pre : 12) : k);
    std::fprintf(stderr, "Serializing SBWT index to %s.sbwt ...\n", prefix.c_str());
    std::fprintf(stderr, "Serializing LCS array to %s.lcs ...\n", prefix.c_str());
    if (ntc_index_save_as(ix, prefix.c_str(), lay)) die("cannot write " + prefix);
    ntc_index_free(ix);
    return 0;
}

void usage(FILE *f) {
    std::fprintf(f,
                 "Sequencing data compression with SBWT + k-bounded matching statistics; encode/decode hot path on "
                 "MI355X.\n\nusage: ntcomp build -o PREFIX [-k K] [-m MEM_GB] [--temp-dir DIR] FILES...\n"
                 "       ntcomp encode -i PREFIX [--non-acgt error|mask|keep] [--exceptions PATH]\n"
                 "                     [--qualities drop|keep|bin8] [--quality-file PATH] [--quality-coder pack|rans]\n"
                 "                     [--quality-smooth [M]] [--quality-smooth-to C]\n"
                 "                     [--names drop|keep|id] [--name-file PATH] [--digest-file PATH]\n"
                 "                     [--deflate auto|zlib|libdeflate|adaptive|gpu] FILE > encoded.dat\n"
                 "                     [--mate-file R2 | --interleaved] [--mate-check ids|off] [--inflate host|gpu]\n"
                 "       ntcomp decode -i PREFIX [--exceptions PATH] [--quality-file PATH] [--name-file PATH]\n"
                 "                     [--digest-file PATH] [--mate-out R2.out] [--reads A-B | --shard I/N] [--bgzf]\n"
                 "                     FILE > out.fasta\n"
                 "       ntcomp verify -i PREFIX --digest-file PATH [--exceptions PATH] [--quality-file PATH]\n"
                 "                     [--name-file PATH] [--reads A-B | --shard I/N] FILE\n"
                 "       ntcomp info [--blocks] FILE\n\n"
                 "  --deflate ENGINE   encode: who gzips the block streams: auto (adaptive when libdeflate.so.0 loads, else\n"
                 "                     zlib), zlib, libdeflate, adaptive, or gpu (on the GPU behind the packer: 32 KiB\n"
                 "                     chunks, greedy in-chunk matches, about 2 %% larger; the host only copies)\n"
                 "  --inflate ENGINE   encode: who inflates a BGZF input: host (default; libdeflate on the reader's threads) or\n"
                 "                     gpu (runs of members inflated on the first GPU; every input must be BGZF; the\n"
                 "                     output is byte for byte the host engine's; not with --host-parse)\n"
                 "  --non-acgt POLICY  encode: reads with N or IUPAC symbols: error (default) stops at the first,\n"
                 "                     mask replaces each symbol by the substitute base (lossy), keep also writes\n"
                 "                     the replaced symbols to the --exceptions file (lossless)\n"
                 "  --exceptions PATH  encode --non-acgt keep: the side file to write; decode: the side file whose\n"
                 "                     symbols are put back\n"
                 "  --qualities MODE   encode: FASTQ quality scores: drop (default), keep (lossless), or bin8 (Phred\n"
                 "                     scores binned to 8 levels, lossy); keep and bin8 write them, packed on the GPU,\n"
                 "                     to the --quality-file\n"
                 "  --quality-file PATH  encode --qualities keep|bin8: the side file to write; decode: the side file\n"
                 "                     whose qualities are printed: the output is then FASTQ\n"
                 "  --quality-coder CODER  encode --qualities keep|bin8: pack (default; packed codes, deflated on the\n"
                 "                     host) or rans (order-1 rANS coded on the GPU, no host deflate)\n"
                 "  --quality-smooth [M]  encode --qualities keep|bin8: smooth the scores inside long matches to the\n"
                 "                     index (lossy): a score above '#' in a long record of at least M bases (12..16777215,\n"
                 "                     32 when M is left out) becomes the --quality-smooth-to byte\n"
                 "  --quality-smooth-to C  the byte --quality-smooth writes: one of '$'..'~' (default I; under bin8\n"
                 "                     above '*')\n"
                 "  --names MODE       encode: FASTQ read names: drop (default), keep (lossless: the header line\n"
                 "                     after '@'), or id (the name up to its first space or tab, lossy); keep and id\n"
                 "                     write them, front-coded on the GPU, to the --name-file\n"
                 "  --name-file PATH   encode --names keep|id: the side file to write; decode: the side file whose\n"
                 "                     names are printed instead of seq.N\n"
                 "  --digest-file PATH encode: also write per-block content digests, computed on the GPU; decode: check\n"
                 "                     every block against them while decoding -- another index, a damaged or truncated\n"
                 "                     file, a side file of another run end the call with an error that names the block\n"
                 "                     and the component; verify: the same check without writing the text\n"
                 "  --mate-file R2     encode: paired-end reads, FILE holds the mate-1 records and R2 the mate-2 records\n"
                 "                     (any supported compression each); the GPU weaves them, read 2p and 2p+1 are a pair\n"
                 "  --interleaved      encode: FILE already alternates the mates\n"
                 "  --mate-check ids|off  encode: compare the mates' ids (cut at the first blank, /1 and /2 stripped)\n"
                 "                     on the GPU (default), or not\n"
                 "  --mate-out R2.out  decode: the archive holds pairs: mate-1 records to stdout, mate-2 records to R2.out\n"
                 "  --reads A-B        decode, verify: only reads A-B of the archive, 1-based and inclusive as decode\n"
                 "                     numbers them (seq.N); also A, A- and -B.  Only the blocks that hold them are read;\n"
                 "                     the reads keep their numbers, names and qualities\n"
                 "  --shard I/N        decode, verify: only the I-th of N contiguous slices of whole blocks; the N outputs\n"
                 "                     concatenated in order are the full decode (one process per GPU or node)\n"
                 "  --bgzf             decode: write the text as BGZF (.gz: bgzip's blocked gzip), cut at record boundaries and\n"
                 "                     compressed on the GPU; with --mate-out both outputs.  The EOF member is written only when\n"
                 "                     the decode succeeds; the --shard outputs concatenated are one BGZF file\n"
                 "  --blocks           info: one line per block\n");
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 2) {
        usage();
        return 2;
    }
    if (std::getenv("NTC_INIT_TRACE")) {  // the wall-clock instant main starts (after the loader)
        struct timespec ts;
        clock_gettime(CLOCK_REALTIME, &ts);
        std::fprintf(stderr, "[init] main at %.6f\n", ts.tv_sec + 1e-9 * ts.tv_nsec);
    }
    const std::string cmd = argv[1];
    if (cmd == "-h" || cmd == "--help" || cmd == "help") {
        usage(stdout);
        return 0;
    }
    if (cmd == "-V" || cmd == "--version") {
        std::printf("ntcomp %s\n", kVersion);
        return 0;
    }
    const Args a = parse(argc, argv, 2);
    if (cmd == "build") return cmd_build(a);
    if (cmd == "info") return cmd_info(a);
    if (cmd == "encode" || cmd == "decode" || cmd == "verify") {
        const int rc = cmd == "encode" ? cmd_encode(a) : cmd_decode(a, cmd == "verify");
        // The output is complete and every device call has returned.  Free the contexts
        // (their device memory: ~15 ms) and leave without the rest of the HIP runtime's
        // teardown.  Exiting with the contexts alive cost more (wall clock after main 0.10-0.13 s
        // against 0.05-0.08 s with them freed first, 10 M-read encode, scripts/exit_cost.py).
        std::fflush(stdout);
        const bool itr = std::getenv("NTC_INIT_TRACE") != nullptr;
        const auto te = Clock::now();
        for (auto *c : g_ctxs) ntc_ctx_destroy(c);
        ntc_index_free(g_ix);
        if (itr) {  // the exit timeline: contexts freed, then the wall-clock instant of _exit
            struct timespec ts;
            clock_gettime(CLOCK_REALTIME, &ts);
            std::fprintf(stderr, "[exit] contexts freed in %.3f ms; _exit at %.6f\n", 1e3 * since(te),
                         ts.tv_sec + 1e-9 * ts.tv_nsec);
        }
        std::fflush(stderr);
        if (std::getenv("NTC_CLEAN_EXIT")) return rc;  // exit handlers run (a profiler writes its trace there)
        _exit(rc);
    }
    usage();
    return 2;
}
