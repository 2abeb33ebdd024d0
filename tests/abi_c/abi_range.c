/* C99 consumer of the range part of the C ABI: includes only the public headers and links
 * libntcomp_gpu.so, so the layout of ntc_file_opts5 / ntc_r_stats / ntc_archive_block is checked
 * by the compiler and the new symbols by the linker (tests/test_range.py). */
#include <stddef.h>
#include <stdio.h>

#include "ntcomp_codec.h"
#include "ntcomp_gpu.h"
#include "ntcomp_pipeline.h"

_Static_assert(sizeof(void *) == 8, "64-bit target");
/* ntc_file_opts4's fields in order, then the two of the range */
_Static_assert(offsetof(ntc_file_opts5, struct_bytes) == offsetof(ntc_file_opts4, struct_bytes) &&
                   offsetof(ntc_file_opts5, nx_policy) == offsetof(ntc_file_opts4, nx_policy) &&
                   offsetof(ntc_file_opts5, nx_fd) == offsetof(ntc_file_opts4, nx_fd) &&
                   offsetof(ntc_file_opts5, q_mode) == offsetof(ntc_file_opts4, q_mode) &&
                   offsetof(ntc_file_opts5, q_fd) == offsetof(ntc_file_opts4, q_fd) &&
                   offsetof(ntc_file_opts5, nx_path) == offsetof(ntc_file_opts4, nx_path) &&
                   offsetof(ntc_file_opts5, q_path) == offsetof(ntc_file_opts4, q_path) &&
                   offsetof(ntc_file_opts5, n_mode) == offsetof(ntc_file_opts4, n_mode) &&
                   offsetof(ntc_file_opts5, n_fd) == offsetof(ntc_file_opts4, n_fd) &&
                   offsetof(ntc_file_opts5, n_path) == offsetof(ntc_file_opts4, n_path) &&
                   offsetof(ntc_file_opts5, d_mode) == offsetof(ntc_file_opts4, d_mode) &&
                   offsetof(ntc_file_opts5, d_fd) == offsetof(ntc_file_opts4, d_fd) &&
                   offsetof(ntc_file_opts5, d_path) == offsetof(ntc_file_opts4, d_path) &&
                   offsetof(ntc_file_opts5, pair_mode) == offsetof(ntc_file_opts4, pair_mode) &&
                   offsetof(ntc_file_opts5, mate_path) == offsetof(ntc_file_opts4, mate_path) &&
                   offsetof(ntc_file_opts5, out_fd2) == offsetof(ntc_file_opts4, out_fd2) && sizeof(ntc_file_opts4) == 96,
               "ntc_file_opts5 starts as ntc_file_opts4");
_Static_assert(offsetof(ntc_file_opts5, read_first) == 96 && offsetof(ntc_file_opts5, read_count) == 104 &&
                   sizeof(ntc_file_opts5) == 112,
               "ntc_file_opts5");
_Static_assert(offsetof(ntc_r_stats, blocks_total) == 0 && offsetof(ntc_r_stats, reads_total) == 8 &&
                   offsetof(ntc_r_stats, first_block) == 16 && offsetof(ntc_r_stats, blocks_read) == 24 &&
                   offsetof(ntc_r_stats, reads_written) == 32 && offsetof(ntc_r_stats, head_skipped) == 40 &&
                   offsetof(ntc_r_stats, tail_skipped) == 48 && sizeof(ntc_r_stats) == 56,
               "ntc_r_stats");
_Static_assert(offsetof(ntc_archive_block, offset) == 0 && offsetof(ntc_archive_block, bytes) == 8 &&
                   offsetof(ntc_archive_block, reads) == 16 && offsetof(ntc_archive_block, records) == 24 &&
                   offsetof(ntc_archive_block, bad) == 32 && sizeof(ntc_archive_block) == 40,
               "ntc_archive_block");

int main(int argc, char **argv) {
    /* every new symbol resolves (the GPU ones are not called: no GPU is needed here) */
    const void *syms[3];
    syms[0] = (const void *)(size_t)&ntc_decode_set_window;
    syms[1] = (const void *)(size_t)&ntc_decode_file_ex5;
    syms[2] = (const void *)(size_t)&ntc_archive_info;
    for (int i = 0; i < 3; i++)
        if (!syms[i]) return 1;
    printf("{\"ntc_file_opts5\": %zu, \"ntc_r_stats\": %zu, \"ntc_archive_block\": %zu}\n", sizeof(ntc_file_opts5),
           sizeof(ntc_r_stats), sizeof(ntc_archive_block));
    if (argc > 1) { /* the host-only call, from C: the archive at argv[1] */
        ntc_archive_block *blocks = NULL;
        uint64_t nb = 0, reads = 0, recs = 0, tail = 0;
        const int rc = ntc_archive_info(argv[1], &blocks, &nb, &reads, &recs, &tail);
        printf("info rc %d blocks %llu reads %llu records %llu tail %llu\n", rc, (unsigned long long)nb,
               (unsigned long long)reads, (unsigned long long)recs, (unsigned long long)tail);
        ntc_buffer_free(blocks);
        return rc;
    }
    return 0;
}
