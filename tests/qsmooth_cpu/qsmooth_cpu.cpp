// The per-read logic of k_q_smooth (quality.hip) on the CPU: the very functions of
// qsmooth_core.h, driven the way the kernel drives them (the records kQsChunk at a time, the
// chunk's qualities an aligned 8-byte word per lane, whole words stored whole and edge words
// byte by byte), built with ASan + UBSan by tests/test_qsmooth.py.
//   qsmooth_cpu IN OUT
// IN : u32 m, u32 mode, u32 to, u32 lead (bytes in front of the first read: the alignment of
//      the array), u32 block_reads, u32 zero, u64 n_reads, u64 n_recs, u64 offs[n_reads + 1],
//      u64 roffs[n_reads + 1], u64 recs[n_recs], the quality bytes (after the mode's table)
// OUT: u64 bytes replaced, u64 n_blocks, per block u64 p0, u64 p1, then the smoothed bytes.
// The program itself checks that no byte outside the reads was written (exit status 3).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../ntcomp_amd/csrc/qsmooth_core.h"

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
    if (!read_all(argv[1], in) || in.size() < 40) return 2;
    uint32_t h[6];
    uint64_t n, n_recs;
    std::memcpy(h, in.data(), 24);
    std::memcpy(&n, in.data() + 24, 8);
    std::memcpy(&n_recs, in.data() + 32, 8);
    const uint32_t m = h[0], mode = h[1], to = h[2], lead = h[3], block_reads = h[4];
    if (lead > 7 || block_reads == 0 || in.size() < 40 + (2 * (n + 1) + n_recs) * 8) return 2;
    std::vector<uint64_t> offs(n + 1), roffs(n + 1), recs(n_recs);
    const uint8_t *at = in.data() + 40;
    std::memcpy(offs.data(), at, (n + 1) * 8);
    std::memcpy(roffs.data(), at += (n + 1) * 8, (n + 1) * 8);
    std::memcpy(recs.data(), at += (n + 1) * 8, n_recs * 8);
    at += n_recs * 8;
    const uint64_t total = offs[n];
    if (in.size() != (uint64_t)(at - in.data()) + total || roffs[n] != n_recs) return 2;

    // the array as the kernel sees it: 8-aligned words, the reads from byte `lead` on, slack behind
    const uint64_t n_words = (lead + total + 64 + 7) / 8;
    std::vector<uint64_t> arr(n_words, 0x7E7E7E7E7E7E7E7Eull);
    uint8_t *quals = (uint8_t *)arr.data();
    std::memcpy(quals + lead, at, total);
    const std::vector<uint64_t> before = arr;

    const uint32_t floor = qs_floor(mode), target = qs_target(mode, to);
    const uint64_t n_blocks = (n + block_reads - 1) / block_reads;
    std::vector<uint64_t> p0(n_blocks, 0), p1(n_blocks, 0);
    uint64_t replaced = 0;
    for (uint64_t r = 0; r < n; r++) {
        const uint64_t o = lead + offs[r], j0 = roffs[r], mrec = roffs[r + 1] - j0, b = r / block_reads;
        uint64_t hi = offs[r + 1] - offs[r];
        for (uint64_t c = 0; c < mrec; c += kQsChunk) {
            const uint32_t cnt = (uint32_t)(mrec - c < kQsChunk ? mrec - c : kQsChunk);
            uint32_t ent[kQsChunk];
            const uint32_t span = qs_chunk_entries(recs.data() + j0 + c, cnt, m, ent);
            if (span > hi) return 4;  // (records that outrun the read)
            if (span == 0) continue;
            const uint64_t lo = o + (hi - span), end = o + hi;
            for (uint64_t w = lo & ~7ull; w < end; w += 8) {  // one lane each
                uint64_t live, changed, word;
                const uint64_t mask = qs_word_mask(ent, cnt, span, (int64_t)w - (int64_t)lo, &live);
                std::memcpy(&word, quals + w, 8);
                const uint64_t v = qs_apply(word, mask, floor, target, &changed);
                qs_presence(v, live, &p0[b], &p1[b]);
                if (changed & ~live) return 3;
                if (!changed) continue;
                replaced += q_popc(changed) >> 3;
                if (live == ~0ull) {
                    std::memcpy(quals + w, &v, 8);
                } else {
                    for (uint32_t j = 0; j < 8; j++)
                        if ((changed >> (8 * j)) & 1) quals[w + j] = (uint8_t)target;
                }
            }
            hi -= span;
        }
        if (hi != 0) return 4;  // the records cover the read
    }
    for (uint64_t i = 0; i < n_words * 8; i++)
        if ((i < lead || i >= lead + total) && quals[i] != ((const uint8_t *)before.data())[i]) return 3;

    std::vector<uint8_t> out;
    put(out, replaced);
    put(out, n_blocks);
    for (uint64_t b = 0; b < n_blocks; b++) {
        put(out, p0[b]);
        put(out, p1[b]);
    }
    out.insert(out.end(), quals + lead, quals + lead + total);
    FILE *f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    const bool ok = std::fwrite(out.data(), 1, out.size(), f) == out.size();
    return std::fclose(f) == 0 && ok ? 0 : 2;
}
