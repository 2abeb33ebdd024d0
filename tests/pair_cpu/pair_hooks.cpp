// The file pipelines without the GPU stage (pipeline.cpp over tests/san/gpu_stub.cpp, no
// capi.cpp): the pairs' hook table stays null, and pair_mode != 0 must answer
// NTC_ERR_UNSUPPORTED before anything is opened; pair_mode 0 must not.  Built and run by
// tests/test_pairs.py.
#include <cstdio>

#include "../../include/ntcomp_gpu.h"
#include "../../include/ntcomp_pipeline.h"

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    ntc_ctx *ctx = reinterpret_cast<ntc_ctx *>(argv);  // never dereferenced before the refusal
    ntc_ctx *const ctxs[1] = {ctx};
    ntc_pipeline_stats st{};
    int bad = 0;
    for (int mode = 1; mode <= 2; mode++) {
        ntc_file_opts4 fo{};
        fo.struct_bytes = sizeof(fo);
        fo.nx_fd = fo.q_fd = fo.n_fd = fo.d_fd = fo.out_fd2 = -1;
        fo.pair_mode = mode;
        const int e = ntc_encode_file_ex4(ctxs, 1, argv[1], 1, &fo, nullptr, &st, nullptr, nullptr, nullptr, nullptr, nullptr);
        fo.out_fd2 = 2;
        const int d = ntc_decode_file_ex4(ctxs, 1, argv[1], 1, &fo, nullptr, &st, nullptr, nullptr);
        std::printf("mode %d: encode %d decode %d\n", mode, e, d);
        bad += e != NTC_ERR_UNSUPPORTED || d != NTC_ERR_UNSUPPORTED;
    }
    ntc_file_opts4 fo{};
    fo.struct_bytes = sizeof(fo) - 8;  // a shorter struct is refused
    const int s = ntc_encode_file_ex4(ctxs, 1, argv[1], 1, &fo, nullptr, &st, nullptr, nullptr, nullptr, nullptr, nullptr);
    std::printf("short struct: %d\n", s);
    bad += s != NTC_ERR_INVALID_ARG;
    return bad ? 1 : 0;
}
