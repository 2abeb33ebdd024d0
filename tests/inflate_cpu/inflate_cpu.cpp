// The inflate decoder of `--inflate gpu` on the CPU: inflate_core.h alone (with the
// deflate_core.h it takes the CRC-32 from), compiled by tests/test_inflate.py under ASan + UBSan
// and run as a child process.
//
//   inflate_cpu IN OUT
// IN holds members back to back: u32 src_bytes, u32 claimed_out (little-endian), then src_bytes
// bytes.  For each member OUT gets u32 status, u32 out_bytes, u32 crc, and under status 0 the
// out_bytes bytes.  Every member is decoded from a buffer of exactly src_bytes bytes into one of
// exactly claimed_out bytes (none above kInfMaxOut: such a member must not touch it), so a
// decoder that reads or writes out of bounds is ended by the sanitizer; a member that fails must
// leave its output buffer as it was.  Python compares with zlib.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../ntcomp_amd/csrc/inflate_core.h"

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
    if (argc != 3) return std::fprintf(stderr, "usage: inflate_cpu IN OUT\n"), 2;
    std::vector<uint8_t> in;
    if (!read_all(argv[1], in)) return std::fprintf(stderr, "cannot read %s\n", argv[1]), 2;
    FILE *out = std::fopen(argv[2], "wb");
    if (!out) return std::fprintf(stderr, "cannot write %s\n", argv[2]), 2;
    ntc::InfWork *W = new ntc::InfWork;  // one working set for every member, as a workgroup's LDS is reused
    std::memset(W, 0xA5, sizeof(*W));
    size_t at = 0;
    int cases = 0;
    while (at < in.size()) {
        uint32_t head[2];
        if (in.size() - at < 8) return std::fprintf(stderr, "short case header\n"), 2;
        std::memcpy(head, in.data() + at, 8);
        at += 8;
        if (in.size() - at < head[0]) return std::fprintf(stderr, "short case\n"), 2;
        std::vector<uint8_t> src(in.begin() + (long)at, in.begin() + (long)(at + head[0]));
        at += head[0];
        std::vector<uint8_t> dst(head[1] <= ntc::kInfMaxOut ? head[1] : 0, 0xC3);
        ntc::InfResult r{99, 99, 99, 99};
        ntc::inf_member(W, src.data(), head[0], head[1], dst.data(), &r, 0, 1);
        if (r.status) {
            for (uint8_t b : dst)
                if (b != 0xC3) return std::fprintf(stderr, "case %d: status %u and the output was written\n", cases, r.status), 1;
        } else if (r.out_bytes != head[1])
            return std::fprintf(stderr, "case %d: status 0 with %u of %u bytes\n", cases, r.out_bytes, head[1]), 1;
        std::fwrite(&r, 4, 3, out);
        if (!r.status && !dst.empty()) std::fwrite(dst.data(), 1, dst.size(), out);
        cases++;
    }
    delete W;
    if (std::fclose(out) != 0) return 2;
    std::printf("%d cases\n", cases);
    return 0;
}
