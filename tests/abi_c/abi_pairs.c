/* C99 consumer of the paired-end part of the C ABI: includes only the public headers and links
 * libntcomp_gpu.so, so the layout of ntc_file_opts4 / ntc_p_stats is checked by the compiler
 * and the new symbols by the linker (tests/test_pairs.py). */
#include <stddef.h>
#include <stdio.h>

#include "ntcomp_codec.h"
#include "ntcomp_gpu.h"
#include "ntcomp_pipeline.h"

_Static_assert(sizeof(void *) == 8, "64-bit target");
/* ntc_file_opts3's fields in order, then the three of the pairs */
_Static_assert(offsetof(ntc_file_opts4, struct_bytes) == offsetof(ntc_file_opts3, struct_bytes) &&
                   offsetof(ntc_file_opts4, nx_path) == offsetof(ntc_file_opts3, nx_path) &&
                   offsetof(ntc_file_opts4, n_path) == offsetof(ntc_file_opts3, n_path) &&
                   offsetof(ntc_file_opts4, d_mode) == offsetof(ntc_file_opts3, d_mode) &&
                   offsetof(ntc_file_opts4, d_path) == offsetof(ntc_file_opts3, d_path) && sizeof(ntc_file_opts3) == 72,
               "ntc_file_opts4 starts as ntc_file_opts3");
_Static_assert(offsetof(ntc_file_opts4, pair_mode) == 72 && offsetof(ntc_file_opts4, mate_path) == 80 &&
                   offsetof(ntc_file_opts4, out_fd2) == 88 && sizeof(ntc_file_opts4) == 96,
               "ntc_file_opts4");
_Static_assert(offsetof(ntc_p_stats, bytes1) == 8 && offsetof(ntc_p_stats, mode) == 24 && sizeof(ntc_p_stats) == 32,
               "ntc_p_stats");

int main(void) {
    /* every new symbol resolves (none is called: no GPU is needed here) */
    const void *syms[4];
    syms[0] = (const void *)(size_t)&ntc_encode_pack_fastq_paired;
    syms[1] = (const void *)(size_t)&ntc_decode_pair_split;
    syms[2] = (const void *)(size_t)&ntc_encode_file_ex4;
    syms[3] = (const void *)(size_t)&ntc_decode_file_ex4;
    for (int i = 0; i < 4; i++)
        if (!syms[i]) return 1;
    printf("{\"ntc_file_opts4\": %zu, \"ntc_p_stats\": %zu}\n", sizeof(ntc_file_opts4), sizeof(ntc_p_stats));
    return 0;
}
