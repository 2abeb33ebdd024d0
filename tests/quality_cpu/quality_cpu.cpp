// The per-lane logic of quality.hip on the CPU: the very functions of quality_core.h, driven
// the way the kernels drive them (gather: table, checks, presence map per block; alphabet;
// pack: 8 qualities per lane, the lanes of one word ORed; unpack: one code per lane), built
// with ASan + UBSan by tests/test_quality.py.
//   quality_cpu IN OUT
// IN : u32 mode, u32 block_reads, u64 n_reads, u64 kept[n_reads] (bases each read keeps),
//      u64 qoff[n_reads + 1], the quality lines' bytes
// OUT: u64 status (~0 = ok, else read << 8 | 8), u64 n_blocks, then per block u64 n_quals,
//      u64 width, u64 n_syms, 96 alphabet bytes, u64 n_words, the words; the program itself
//      checks that unpacking the words gives the table's bytes back (exit status 3 if not).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../ntcomp_amd/csrc/quality_core.h"

using namespace ntc;

static bool read_all(const char *path, std::vector<uint8_t> &buf) {
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    uint8_t chunk[1 << 16];
    size_t got;
    while ((got = std::fread(chunk, 1, sizeof(chunk), f)) > 0) buf.insert(buf.end(), chunk, chunk + got);
    std::fclose(f);
    return true;
}

template <class T>
static void put(std::vector<uint8_t> &o, const T &v) {
    const uint8_t *p = (const uint8_t *)&v;
    o.insert(o.end(), p, p + sizeof(T));
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    std::vector<uint8_t> in;
    if (!read_all(argv[1], in) || in.size() < 16) return 2;
    uint32_t mode, block_reads;
    uint64_t n;
    std::memcpy(&mode, in.data(), 4);
    std::memcpy(&block_reads, in.data() + 4, 4);
    std::memcpy(&n, in.data() + 8, 8);
    if (block_reads == 0 || in.size() < 16 + (2 * n + 1) * 8) return 2;
    std::vector<uint64_t> kept(n), qoff(n + 1);
    std::memcpy(kept.data(), in.data() + 16, n * 8);
    std::memcpy(qoff.data(), in.data() + 16 + n * 8, (n + 1) * 8);
    const uint8_t *raw = in.data() + 16 + (2 * n + 1) * 8;
    if (in.size() != 16 + (2 * n + 1) * 8 + qoff[n]) return 2;

    uint64_t status = ~0ull;
    const uint64_t n_blocks = (n + block_reads - 1) / block_reads;
    std::vector<uint8_t> out;
    std::vector<std::vector<uint8_t>> quals(n_blocks);
    std::vector<uint64_t> p0(n_blocks, 0), p1(n_blocks, 0);
    // gather
    for (uint64_t r = 0; r < n; r++) {
        const uint64_t b = r / block_reads, len = qoff[r + 1] - qoff[r];
        bool bad = len != kept[r];
        for (uint64_t i = 0; i < len && !bad; i++) {
            const uint32_t t = q_table(mode, raw[qoff[r] + i]);
            if (!t) {
                bad = true;
                break;
            }
            quals[b].push_back((uint8_t)t);
            (t < 64 ? p0[b] : p1[b]) |= 1ull << (t & 63);
        }
        if (bad) {
            const uint64_t v = r << 8 | 8;
            if (v < status) status = v;
        }
    }
    put(out, status);
    put(out, n_blocks);
    if (status == ~0ull) {
        for (uint64_t b = 0; b < n_blocks; b++) {
            uint8_t alphabet[96] = {0};
            const uint64_t nq = quals[b].size();
            const uint64_t n_syms = q_alphabet(p0[b], p1[b], alphabet), w = q_width((uint32_t)n_syms);
            const uint64_t nw = q_words(nq, (uint32_t)w);
            std::vector<uint64_t> words(nw, 0);
            if (w) {  // lane l of a group packs qualities [8 l, 8 l + 8); 8 / w lanes share a word
                const uint32_t per = 8 / (uint32_t)w;
                for (uint64_t i = 0, lane = 0; i < nq; i += 8, lane++) {
                    uint64_t v = 0;
                    const uint32_t live = (uint32_t)(nq - i < 8 ? nq - i : 8);
                    std::memcpy(&v, quals[b].data() + i, live);
                    v |= live < 8 ? 0x5A5A5A5A5A5A5A5Aull << (8 * live) : 0;  // bytes past the block: any
                    words[i * w >> 6] |= q_pack8(v, live, p0[b], p1[b], (uint32_t)w) << ((lane % per) * 8 * w);
                }
                for (uint64_t i = 0; i < nq; i++) {
                    const uint32_t c = q_code_at(words.data(), i, (uint32_t)w);
                    if (c >= n_syms || alphabet[c] != quals[b][i]) return 3;
                }
            } else if (nq) {
                for (uint64_t i = 0; i < nq; i++)
                    if (alphabet[0] != quals[b][i]) return 3;
            }
            if (!q_meta_ok(nq, (uint32_t)w, (uint32_t)n_syms, alphabet)) return 3;
            put(out, nq);
            put(out, w);
            put(out, n_syms);
            out.insert(out.end(), alphabet, alphabet + 96);
            put(out, nw);
            for (uint64_t x : words) put(out, x);
        }
    }
    FILE *f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    const bool ok = std::fwrite(out.data(), 1, out.size(), f) == out.size();
    return std::fclose(f) == 0 && ok ? 0 : 2;
}
