// names_core.h on the CPU: the functions the kernels of ntcomp_amd/csrc/names.hip call, walked
// the way the kernels walk them (a "wave" of 64 lanes per name, comparisons in 64-byte steps
// whose agreement masks are built lane by lane), so that ASan + UBSan see the cut, prefix,
// suffix, section and expansion logic.  tests/test_names.py builds it with
// -fsanitize=address,undefined and compares its output with names_lib.py.
//
//   names_cpu IN OUT
// IN:  u32 mode, u32 block_reads, u64 n, then per read u32 bytes + its header line ('@' first,
//      no newline, a trailing '\r' still on it)
// OUT: u64 status (~0: fine, else read << 8 | 8), u64 blocks, then per block its five u64
//      (n_reads, name_bytes, mid_bytes, payload_off, payload_bytes) and its payload bytes;
//      the program exits 3 if expanding a section does not give the names back.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../ntcomp_amd/csrc/names_core.h"

using namespace ntc;

namespace {

using Bytes = std::vector<uint8_t>;

// k_n_measure's n_span: the name inside its header line
void span_of(const Bytes &line, uint32_t mode, uint64_t &s, uint64_t &len) {
    s = line.empty() ? 0 : 1;
    len = line.size() - s;
    if (len && line[line.size() - 1] == '\r') len--;
    if (mode == kNId) {
        for (uint64_t b = 0; b < len; b += 64) {
            uint64_t m = 0;
            for (uint32_t lane = 0; lane < 64; lane++)
                if (b + lane < len && n_is_cut(line[s + b + lane])) m |= 1ull << lane;
            if (m) {
                len = b + n_ctz(m);
                break;
            }
        }
    }
}

bool read_all(const char *path, Bytes &out) {
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    uint8_t chunk[1 << 16];
    size_t got;
    while ((got = std::fread(chunk, 1, sizeof(chunk), f)) > 0) out.insert(out.end(), chunk, chunk + got);
    std::fclose(f);
    return true;
}

void put64(Bytes &o, uint64_t v) {
    for (int i = 0; i < 8; i++) o.push_back((uint8_t)(v >> (8 * i)));
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    Bytes in;
    if (!read_all(argv[1], in) || in.size() < 16) return 2;
    uint32_t mode, block_reads;
    uint64_t n;
    std::memcpy(&mode, in.data(), 4);
    std::memcpy(&block_reads, in.data() + 4, 4);
    std::memcpy(&n, in.data() + 8, 8);
    std::vector<Bytes> lines(n);
    size_t at = 16;
    for (uint64_t r = 0; r < n; r++) {
        uint32_t len;
        if (in.size() - at < 4) return 2;
        std::memcpy(&len, in.data() + at, 4);
        at += 4;
        if (in.size() - at < len) return 2;
        lines[r].assign(in.begin() + at, in.begin() + at + len);
        at += len;
    }
    // measure
    uint64_t status = ~0ull;
    std::vector<uint64_t> start(n), len(n);
    std::vector<uint32_t> pre(n), suf(n);
    for (uint64_t r = 0; r < n; r++) {
        span_of(lines[r], mode, start[r], len[r]);
        if (len[r] > kNMax) {
            const uint64_t code = r << 8 | 8;
            if (code < status) status = code;
            len[r] = 0;
            continue;
        }
        if ((r % block_reads) % kNGroup == 0) continue;
        uint64_t ps, pl;
        span_of(lines[r - 1], mode, ps, pl);
        const uint32_t plen = (uint32_t)(pl < kNMax ? pl : kNMax), l = (uint32_t)len[r];
        const uint8_t *P = lines[r - 1].data() + ps, *N = lines[r].data() + start[r];
        const uint32_t lim = n_pre_limit(plen, l);
        for (uint32_t b = 0; b < lim; b += 64) {
            const uint32_t live = lim - b < 64 ? lim - b : 64;
            uint64_t eq = 0;
            for (uint32_t lane = 0; lane < 64; lane++)
                if (lane < live && P[b + lane] == N[b + lane]) eq |= 1ull << lane;
            const uint32_t k = n_run(eq, live);
            pre[r] += k;
            if (k < live) break;
        }
        const uint32_t slim = n_suf_limit(plen, l, pre[r]);
        for (uint32_t b = 0; b < slim; b += 64) {
            const uint32_t live = slim - b < 64 ? slim - b : 64;
            uint64_t eq = 0;
            for (uint32_t lane = 0; lane < 64; lane++)
                if (lane < live && P[plen - 1 - b - lane] == N[l - 1 - b - lane]) eq |= 1ull << lane;
            const uint32_t k = n_run(eq, live);
            suf[r] += k;
            if (k < live) break;
        }
    }
    Bytes out;
    put64(out, status);
    const uint64_t nb = status == ~0ull ? (n + block_reads - 1) / block_reads : 0;
    put64(out, nb);
    uint64_t off = 0;
    for (uint64_t b = 0; b < nb; b++) {
        const uint64_t r0 = b * block_reads, r1 = r0 + block_reads < n ? r0 + block_reads : n, m = r1 - r0;
        uint64_t name_bytes = 0, mid_bytes = 0;
        for (uint64_t r = r0; r < r1; r++) {
            name_bytes += len[r];
            mid_bytes += len[r] - pre[r] - suf[r];
        }
        const uint64_t bytes = n_payload_bytes(m, mid_bytes);
        Bytes sec(bytes, 0xEE);  // (every byte must be written below)
        uint64_t mo = 4 * m;
        for (uint64_t r = r0; r < r1; r++) {
            const uint64_t i = r - r0;
            sec[2 * i] = (uint8_t)len[r];
            sec[2 * i + 1] = (uint8_t)(len[r] >> 8);
            sec[2 * m + i] = (uint8_t)pre[r];
            sec[3 * m + i] = (uint8_t)suf[r];
            for (uint64_t j = 0; j < len[r] - pre[r] - suf[r]; j++) sec[mo++] = lines[r][start[r] + pre[r] + j];
        }
        while (mo < bytes) sec[mo++] = 0;
        // expand it again as k_n_expand does: the previous name in one buffer, this one in the other
        Bytes buf[2] = {Bytes(kNMax + 1), Bytes(kNMax + 1)};
        uint32_t plen = 0, cur = 0;
        uint64_t mid_at = 4 * m;
        for (uint64_t i = 0; i < m; i++, cur ^= 1) {
            const uint32_t l = (uint32_t)sec[2 * i] | (uint32_t)sec[2 * i + 1] << 8, p = sec[2 * m + i], s = sec[3 * m + i];
            if (!n_read_ok((uint32_t)(i % kNGroup), l, p, s, plen)) return 3;
            for (uint32_t j = 0; j < l; j++)
                buf[cur][j] = n_byte(buf[cur ^ 1].data(), plen, sec.data() + mid_at, l, p, s, j);
            if (l != len[r0 + i] || std::memcmp(buf[cur].data(), lines[r0 + i].data() + start[r0 + i], l) != 0) return 3;
            mid_at += l - p - s;
            plen = l;
        }
        put64(out, m);
        put64(out, name_bytes);
        put64(out, mid_bytes);
        put64(out, off);
        put64(out, bytes);
        out.insert(out.end(), sec.begin(), sec.end());
        off += bytes;
    }
    FILE *f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    const bool ok = std::fwrite(out.data(), 1, out.size(), f) == out.size();
    return std::fclose(f) == 0 && ok ? 0 : 2;
}
