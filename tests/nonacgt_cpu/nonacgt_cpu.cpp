// The lane logic of nonacgt.hip on the CPU (tests/test_nonacgt.py builds this with
// -fsanitize=address,undefined and runs it): the same nonacgt_core.h functions the kernels
// call, driven by loops shaped like the kernels -- one iteration per chunk, per read, per
// word, per run.  Input: a file of bases and a file of u64 read offsets (n_reads + 1,
// absolute into the bases; offs[0] may be non-zero), and the substitute base.  Output: one
// "read pos len sym" line per run, then "masked " + the batch's bases after substitution.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../ntcomp_amd/csrc/nonacgt_core.h"

using namespace ntc;

static std::vector<uint8_t> slurp(const char *path) {
    std::vector<uint8_t> v;
    FILE *f = std::fopen(path, "rb");
    if (!f) return v;
    uint8_t buf[4096];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) v.insert(v.end(), buf, buf + n);
    std::fclose(f);
    return v;
}

int main(int argc, char **argv) {
    if (argc != 4) {
        std::fprintf(stderr, "usage: nonacgt_cpu BASES OFFSETS SUB\n");
        return 2;
    }
    std::vector<uint8_t> bases = slurp(argv[1]);
    const std::vector<uint8_t> ob = slurp(argv[2]);
    const uint32_t sub = (uint8_t)argv[3][0];
    if (ob.size() < 16 || ob.size() % 8) return 2;
    std::vector<uint64_t> offs(ob.size() / 8);
    std::memcpy(offs.data(), ob.data(), ob.size());
    const uint64_t n_reads = offs.size() - 1, total = offs[n_reads] - offs[0], W = (total + 63) / 64;
    if (offs[n_reads] > bases.size()) return 2;
    const uint8_t *B = bases.data() + offs[0];
    // exactly W words: a chunk or word index one too far is an ASan report
    std::vector<uint64_t> M(W), S(W), E(W), soff(W + 1), eoff(W + 1);
    uint16_t *M16 = (uint16_t *)M.data(), *S16 = (uint16_t *)S.data(), *E16 = (uint16_t *)E.data();
    // k_nx_flag
    for (uint64_t t = 0; t < 4 * W; t++) {
        const uint64_t x0 = t * 16;
        NxFlags f{0, 0, 0};
        if (x0 < total) {
            const uint32_t n = total - x0 < 16 ? (uint32_t)(total - x0) : 16u;
            uint32_t w[4] = {0, 0, 0, 0};
            for (uint32_t j = 0; j < n; j++) w[j >> 2] |= (uint32_t)B[x0 + j] << (8 * (j & 3));
            f = nx_chunk_flags(w, n, kNxNone, kNxNone);
            if (f.m) {
                const uint32_t prev = x0 ? B[x0 - 1] : kNxNone;
                const uint32_t next = x0 + 16 < total ? B[x0 + 16] : kNxNone;
                f = nx_chunk_flags(w, n, prev, next);
            }
        }
        M16[t] = (uint16_t)f.m;
        S16[t] = (uint16_t)f.s;
        E16[t] = (uint16_t)f.e;
    }
    // k_nx_bounds
    for (uint64_t r = 0; r < n_reads; r++) {
        const uint64_t p = offs[r] - offs[0], q = offs[r + 1] - offs[0];
        if (q <= p || q > total) continue;
        if (nx_bit(M.data(), p)) S[p >> 6] |= 1ull << (p & 63);
        if (nx_bit(M.data(), q - 1)) E[(q - 1) >> 6] |= 1ull << ((q - 1) & 63);
    }
    // k_nx_count + the scans
    soff[0] = eoff[0] = 0;
    for (uint64_t w = 0; w < W; w++) {
        soff[w + 1] = soff[w] + (uint64_t)__builtin_popcountll(S[w]);
        eoff[w + 1] = eoff[w] + (uint64_t)__builtin_popcountll(E[w]);
    }
    if (soff[W] != eoff[W]) {
        std::printf("unpaired %llu %llu\n", (unsigned long long)soff[W], (unsigned long long)eoff[W]);
        return 1;
    }
    // k_nx_emit
    for (uint64_t i = 0; i < soff[W]; i++) {
        NxRun r;
        if (!nx_emit_run(i, S.data(), E.data(), soff.data(), eoff.data(), W, bases.data(), offs.data(), n_reads, r)) {
            std::printf("overflow\n");
            return 1;
        }
        std::printf("%llu %u %u %u\n", (unsigned long long)r.read, r.pos, r.len, r.sym);
    }
    // k_nx_substitute
    for (uint64_t t = 0; t < 4 * W; t++)
        for (uint32_t m = M16[t]; m; m &= m - 1) bases[offs[0] + t * 16 + (uint32_t)__builtin_ctz(m)] = (uint8_t)sub;
    std::printf("masked ");
    std::fwrite(bases.data() + offs[0], 1, total, stdout);
    std::printf("\n");
    return 0;
}
