// The text window's rule (ntcomp_amd/csrc/window_core.h) on the CPU: the very functions the
// kernels of window.hip and the windowed writers call, compiled with a host compiler (under
// ASan + UBSan by tests/test_range.py) and walked the way the kernels walk them.
//
//   window_cpu IN OUT
// IN:  u64 n, first, count, paired; u64 sizes[n] (each read's record bytes in the whole
//      batch's text); the text (sum of the sizes)
// OUT: u64 valid; when valid: u64 total (the window's bytes); the window's text
//
//   sizes   k_window_sizes: thread t of n - count zeroes the t-th read outside the window
//   scan    an exclusive scan of the sizes (n + 1 offsets)
//   write   a writer skips read r when w_skips(off[r], off[r + 1]); else it copies the record
//           to off[r], as k_fasta / k_fastq / k_named place it
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../ntcomp_amd/csrc/window_core.h"

static std::vector<uint8_t> slurp(const char *path) {
    std::vector<uint8_t> v;
    FILE *f = std::fopen(path, "rb");
    if (!f) return v;
    uint8_t buf[1 << 16];
    size_t k;
    while ((k = std::fread(buf, 1, sizeof(buf), f)) > 0) v.insert(v.end(), buf, buf + k);
    std::fclose(f);
    return v;
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    const std::vector<uint8_t> in = slurp(argv[1]);
    if (in.size() < 32) return 2;
    uint64_t head[4];
    std::memcpy(head, in.data(), 32);
    const uint64_t n = head[0], first = head[1], count = head[2];
    const bool paired = head[3] != 0;
    if (in.size() < 32 + 8 * n) return 2;
    std::vector<uint64_t> sizes(n), src(n + 1, 0);
    if (n) std::memcpy(sizes.data(), in.data() + 32, 8 * n);
    for (uint64_t r = 0; r < n; r++) src[r + 1] = src[r] + sizes[r];
    const uint8_t *text = in.data() + 32 + 8 * n;
    if (in.size() != 32 + 8 * n + src[n]) return 2;

    FILE *out = std::fopen(argv[2], "wb");
    if (!out) return 2;
    const uint64_t valid = ntc::w_valid(first, count, n, paired) ? 1 : 0;
    std::fwrite(&valid, 8, 1, out);
    if (!valid) return std::fclose(out) ? 2 : 0;

    // k_window_sizes: one thread per read outside the window
    std::vector<uint64_t> win = sizes;
    for (uint64_t t = 0; t < n - count; t++) {
        const uint64_t r = t < first ? t : t + count;
        if (r >= n) return 3;  // the grid covers exactly the reads outside
        if (!ntc::w_keeps(r, first, count)) win[r] = 0;
    }
    for (uint64_t r = 0; r < n; r++)
        if (win[r] != ntc::w_size(sizes[r], r, first, count)) return 3;  // both statements of the rule agree
    std::vector<uint64_t> off(n + 1, 0);
    for (uint64_t r = 0; r < n; r++) off[r + 1] = off[r] + win[r];
    std::vector<uint8_t> dst(off[n]);
    uint64_t written = 0;
    for (uint64_t r = 0; r < n; r++) {
        if (ntc::w_skips(off[r], off[r + 1])) continue;
        if (off[r] + sizes[r] > dst.size()) return 3;
        std::memcpy(dst.data() + off[r], text + src[r], sizes[r]);
        written += sizes[r];
    }
    if (written != off[n]) return 3;
    std::fwrite(&off[n], 8, 1, out);
    if (!dst.empty()) std::fwrite(dst.data(), 1, dst.size(), out);
    return std::fclose(out) ? 2 : 0;
}
