// The deflate coder of `--deflate gpu` on the CPU: deflate_core.h alone, compiled by
// tests/test_deflate_gpu_host.py under ASan + UBSan and run as a child process.
//
//   deflate_cpu IN OUT
// IN holds cases back to back: u64 n (little-endian), then n bytes.  For each case OUT gets
// u64 member bytes, u64 chunks, the chunks' encodings (1, 2 or 3, a byte each), the member.
// The member's buffer is exactly df_member_bound(n) bytes, so a coder that passes its bound
// writes out of bounds and the sanitizer ends the run; every case is coded twice and the two
// results must be the same bytes.  Python inflates the members.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../ntcomp_amd/csrc/deflate_core.h"

static bool read_all(const char *path, std::vector<uint8_t> &buf) {
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    uint8_t chunk[1 << 16];
    size_t got;
    while ((got = std::fread(chunk, 1, sizeof(chunk), f)) > 0) buf.insert(buf.end(), chunk, chunk + got);
    std::fclose(f);
    return true;
}

int main(int argc, char **argv) {
    if (argc != 3) return std::fprintf(stderr, "usage: deflate_cpu IN OUT\n"), 2;
    std::vector<uint8_t> in;
    if (!read_all(argv[1], in)) return std::fprintf(stderr, "cannot read %s\n", argv[1]), 2;
    FILE *out = std::fopen(argv[2], "wb");
    if (!out) return std::fprintf(stderr, "cannot write %s\n", argv[2]), 2;
    size_t at = 0;
    int cases = 0;
    while (at < in.size()) {
        uint64_t n = 0;
        if (in.size() - at < 8) return std::fprintf(stderr, "short case header\n"), 2;
        std::memcpy(&n, in.data() + at, 8);
        at += 8;
        if (in.size() - at < n) return std::fprintf(stderr, "short case\n"), 2;
        // the case in a buffer of its own size, so a read past its end is seen
        std::vector<uint8_t> data(in.begin() + (long)at, in.begin() + (long)(at + n));
        at += n;
        const uint64_t bound = ntc::df_member_bound(n), nc = ntc::df_chunks(n);
        std::vector<uint8_t> a(bound), b(bound), ca(nc), cb(nc);
        const uint64_t la = ntc::df_member_host(data.data(), n, a.data(), ca.data());
        const uint64_t lb = ntc::df_member_host(data.data(), n, b.data(), cb.data());
        if (la > bound) return std::fprintf(stderr, "case %d: %llu bytes pass the bound %llu\n", cases,
                                            (unsigned long long)la, (unsigned long long)bound), 1;
        if (la != lb || std::memcmp(a.data(), b.data(), la) != 0 || ca != cb)
            return std::fprintf(stderr, "case %d: two runs differ\n", cases), 1;
        std::fwrite(&la, 8, 1, out);
        std::fwrite(&nc, 8, 1, out);
        std::fwrite(ca.data(), 1, nc, out);
        std::fwrite(a.data(), 1, la, out);
        cases++;
    }
    if (std::fclose(out) != 0) return 2;
    std::printf("%d cases\n", cases);
    return 0;
}
