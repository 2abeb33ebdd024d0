// The BGZF member plan and coder on the CPU: bgzf_core.h and deflate_core.h alone, compiled by
// tests/test_bgzf.py under ASan + UBSan and run as a child process.
//
//   bgzf_cpu IN OUT
// IN holds cases back to back: u64 n, u64 offsets (0: none), n bytes of text, the offsets as
// u64 (all little-endian).  For each case OUT gets u64 members, u64 bytes, the member table
// (32 bytes an entry), the members.  The text, the offsets and the output live in buffers of
// exactly their sizes (the output: bgzf_bound(n)), so a read or write past an end is seen by the
// sanitizer; every case runs twice and the two results must be the same bytes.  Python checks
// the members.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../ntcomp_amd/csrc/bgzf_core.h"

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
    if (argc != 3) return std::fprintf(stderr, "usage: bgzf_cpu IN OUT\n"), 2;
    std::vector<uint8_t> in;
    if (!read_all(argv[1], in)) return std::fprintf(stderr, "cannot read %s\n", argv[1]), 2;
    FILE *out = std::fopen(argv[2], "wb");
    if (!out) return std::fprintf(stderr, "cannot write %s\n", argv[2]), 2;
    size_t at = 0;
    int cases = 0;
    while (at < in.size()) {
        uint64_t head[2];
        if (in.size() - at < 16) return std::fprintf(stderr, "short case header\n"), 2;
        std::memcpy(head, in.data() + at, 16);
        at += 16;
        const uint64_t n = head[0], n_off = head[1];
        if (in.size() - at < n + 8 * n_off) return std::fprintf(stderr, "short case\n"), 2;
        std::vector<uint8_t> text(in.begin() + (long)at, in.begin() + (long)(at + n));
        at += n;
        std::vector<uint64_t> off(n_off);
        if (n_off) std::memcpy(off.data(), in.data() + at, 8 * n_off);
        at += 8 * n_off;
        const uint64_t bound = ntc::bgzf_bound(n);
        std::vector<uint8_t> a(bound), b(bound);
        std::vector<ntc::BgzfMember> ta, tb;
        uint64_t ca[7] = {0, 0, 0, 0, 0, 0, 0}, cb[7] = {0, 0, 0, 0, 0, 0, 0};
        ntc::bgzf_host(text.data(), n, n_off ? off.data() : nullptr, n_off ? n_off - 1 : 0, a.data(), ta, ca);
        ntc::bgzf_host(text.data(), n, n_off ? off.data() : nullptr, n_off ? n_off - 1 : 0, b.data(), tb, cb);
        if (ca[3] > bound || ta.size() > ntc::bgzf_members_max(n))
            return std::fprintf(stderr, "case %d: %llu bytes in %zu members pass the bound\n", cases, (unsigned long long)ca[3], ta.size()), 1;
        if (std::memcmp(ca, cb, sizeof(ca)) != 0 || (ca[3] && std::memcmp(a.data(), b.data(), ca[3]) != 0) || ta.size() != tb.size() ||
            (ta.size() && std::memcmp(ta.data(), tb.data(), ta.size() * sizeof(ntc::BgzfMember)) != 0))
            return std::fprintf(stderr, "case %d: two runs differ\n", cases), 1;
        if (ca[0] != ta.size() || ca[1] != ca[4] + ca[5] + ca[6] || ca[2] != n)
            return std::fprintf(stderr, "case %d: the counts do not add up\n", cases), 1;
        for (const ntc::BgzfMember &m : ta)  // BSIZE is a u16: no member passes 65,536 bytes
            if (m.bytes > 65536 || m.text_bytes > ntc::kBgzfMember || m.bytes > m.text_bytes + ntc::kBgzfSlack)
                return std::fprintf(stderr, "case %d: a member of %llu bytes\n", cases, (unsigned long long)m.bytes), 1;
        const uint64_t nm = ta.size();
        std::fwrite(&nm, 8, 1, out);
        std::fwrite(&ca[3], 8, 1, out);
        if (nm) std::fwrite(ta.data(), sizeof(ntc::BgzfMember), nm, out);
        if (ca[3]) std::fwrite(a.data(), 1, ca[3], out);
        cases++;
    }
    if (std::fclose(out) != 0) return 2;
    std::printf("%d cases\n", cases);
    return 0;
}
