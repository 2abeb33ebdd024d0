// TEST-ONLY stand-alone program (tests/test_uniq_hint.py builds it with the address and
// undefined-behaviour sanitizers and runs it): the run-length code derived.cpp build_paths
// writes into colex_at, held against its definition evaluated bit by bit from puniq.
//   uniq_hint_cpu INDEX   INDEX = {n, k, C[4]} as u64, 4 rows of ceil(n / 64) u64, n bytes of LCS
// Prints "codes: c0 c1 c2 c3" (node words per code) and returns 0, or says what differs.
//   uniq_hint_cpu         (no argument) EntryView::run_from on made-up run entries: for every
// distance of the first clear puniq bit below the record end, every cap and every place of the
// entry's first d = k position, the count with the code equals the count without it.  On a
// real cover a clear bit inside a path needs a linked branch, so reads rarely put one next to
// a threshold; here every combination is made.  Prints "sweep: N calls, M with a code".
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../ntcomp_amd/csrc/derived.h"

using namespace ntc;

static int fail(const char *what, uint64_t j);
namespace {
bool read_all(FILE *f, void *p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

}  // namespace
static int fail(const char *what, uint64_t j) {
    printf("FAIL %s at text position %llu\n", what, (unsigned long long)j);
    return 1;
}

// Two run entries over a text of two paths: entry 0 = read [0, p1) at text v0, entry 1 = read
// [p1, len) at text v1; one clear puniq bit `gap` positions below the text position of x + 1
// (gap = 0: none in reach), codes by the definition.
static int sweep() {
    const uint32_t k = 9, len = 420, tlen = 2048;
    std::vector<uint64_t> puniq(tlen / 64 + 4);
    std::vector<uint32_t> colex(tlen + 8);
    uint64_t calls = 0, decided = 0;
    for (uint32_t p1 : {0u, 1u, 40u, 200u}) {
        for (uint32_t d1 : {1u, 5u, 9u}) {  // d at entry 1's first position: its first d = k position moves
            const uint32_t v0 = 300, v1 = 1000;
            Entry E[2] = {{0, v0, p1, kRunTag | 9u}, {p1, v1, len - p1, kRunTag | d1}};
            const int ne = p1 ? 2 : 1;
            if (!p1) E[0] = E[1];
            for (uint32_t X : {11u, 12u, 33u, 41u, 42u, 50u, 73u, 105u, 137u, 170u, 201u, 202u, 233u, 265u, 340u, 419u}) {
                if (X < p1) continue;  // X: the record end in entry 1; run_from starts at X - 1
                const uint32_t jx = v1 + (X - p1);
                for (uint32_t gap = 0; gap <= 140; gap++) {
                    for (auto &w : puniq) w = ~0ull;
                    if (gap) puniq[(jx - gap) >> 6] &= ~(1ull << ((jx - gap) & 63));
                    puniq[(v1 - 1) >> 6] &= ~(1ull << ((v1 - 1) & 63));  // the pad below each path
                    puniq[(v0 - 1) >> 6] &= ~(1ull << ((v0 - 1) & 63));
                    uint32_t r = 0;  // the definition, bit by bit
                    while (r < 200 && ((puniq[(jx - 1 - r) >> 6] >> ((jx - 1 - r) & 63)) & 1u)) r++;
                    colex[jx] = jx | 1u << 31 | (r >= 128 ? 3u : (r >= 64 ? 2u : (r >= 32 ? 1u : 0u))) << kUniqShift;
                    DevIndex ix{};
                    ix.k = k;
                    ix.tab_u = 4;  // (!= k: an uncovered position ends the count)
                    ix.puniq = puniq.data();
                    ix.colex_at = colex.data();
                    ix.uniq_hint = 1;
                    ix.node_mask = kNodeMaskHint;
                    for (uint32_t cap = 1; cap <= X - 1 && cap <= 140; cap++) {
                        EntryView ev(E, &ix, nullptr, 0, k, ne - 1);
                        uint32_t d, sx;
                        ev.DS(X, d, sx);
                        if (d != k) break;  // (the parse tests only below a d = k record end)
                        if ((sx & kNodeMaskHint) != (jx & kNodeMaskHint)) return fail("sweep: S", X);
                        const uint32_t with = ev.run_from(X - 1, cap, sx), without = ev.run_from(X - 1, cap, 0);
                        if (with != without) {
                            printf("FAIL sweep: p1=%u d1=%u X=%u gap=%u cap=%u: %u with the code, %u without\n", p1, d1,
                                   X, gap, cap, with, without);
                            return 1;
                        }
                        calls++;
                        decided += (sx >> kUniqShift) & 3u ? 1 : 0;
                    }
                }
            }
        }
    }
    printf("sweep: %llu calls, %llu with a code\n", (unsigned long long)calls, (unsigned long long)decided);
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 1) return sweep();
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t head[6];
    HostIndex hx;
    if (!read_all(f, head, sizeof head)) return 2;
    hx.n = head[0];
    hx.k = (uint32_t)head[1];
    const uint64_t nw = (hx.n + 63) / 64;
    for (int c = 0; c < 4; c++) {
        hx.C[c] = head[2 + c];
        hx.rows[c].resize(nw);
        if (!read_all(f, hx.rows[c].data(), nw * 8)) return 2;
    }
    hx.lcs.resize(hx.n);
    if (!read_all(f, hx.lcs.data(), hx.n)) return 2;
    fclose(f);
    hx.lcs.resize(hx.n + 256, 0);

    Derived dv;
    std::string err;
    if (!build_derived(hx, dv, err, true)) {  // the cover with the code (the default)
        printf("FAIL build_derived: %s\n", err.c_str());
        return 1;
    }
    if (!dv.has_paths || !dv.uniq_hint) return fail("no cover or no code", 0);
    Derived plain = dv, forced = dv;
    build_paths(hx, plain, false);       // switched off
    build_paths(hx, forced, true, 0);    // on, but the n <= 2^29 rule says no
    if (plain.uniq_hint || forced.uniq_hint) return fail("uniq_hint set without the code", 0);
    if (plain.colex_at.size() != dv.colex_at.size() || plain.tlen != dv.tlen) return fail("cover size", 0);
    if (forced.colex_at != plain.colex_at) return fail("bits set with the rule forced off", 0);
    if (plain.puniq != dv.puniq || plain.pos_of_node != dv.pos_of_node) return fail("puniq / pos_of_node changed", 0);

    const uint32_t k = hx.k;
    const uint32_t code_bits = 3u << kUniqShift;
    uint64_t count[4] = {0, 0, 0, 0};
    for (uint64_t j = 0; j < dv.colex_at.size(); j++) {
        const uint32_t w = dv.colex_at[j], p = plain.colex_at[j];
        bool valid = false;  // a node's k-mer starts at j: a k-mer ends at j + k - 1
        if (j < dv.tlen) {
            const uint64_t end = j + k - 1;
            valid = (dv.pstream[end >> 5].z >> (end & 31)) & 1u;
        }
        if (!valid) {
            if (w != p) return fail("a slot without a node changed", j);
            continue;
        }
        if ((p & code_bits) != 0 || (p & kNodeMaskHint) >= hx.n) return fail("node does not fit below the code", j);
        if ((w & ~code_bits) != p) return fail("node or uniq bit changed", j);
        if ((w & kNodeMaskHint) != (p & kNodeMaskPlain)) return fail("node & mask changed", j);
        if (dv.pos_of_node[w & kNodeMaskHint] != j) return fail("pos_of_node disagrees", j);
        if (((w >> 31) & 1u) != ((dv.puniq[j >> 6] >> (j & 63)) & 1u)) return fail("uniq bit against puniq", j);
        uint32_t r = 0;  // the definition: set puniq bits at j - 1, j - 2, ...
        for (uint64_t t = j; t > 0 && r < 200 && ((dv.puniq[(t - 1) >> 6] >> ((t - 1) & 63)) & 1u); t--) r++;
        const uint32_t want = r >= 128 ? 3u : (r >= 64 ? 2u : (r >= 32 ? 1u : 0u));
        if (((w >> kUniqShift) & 3u) != want) return fail("code", j);
        if (j > 0 && ones_down(dv.puniq.data(), (uint32_t)(j - 1), 200) != r) return fail("ones_down", j);
        count[want]++;
    }
    printf("codes: %llu %llu %llu %llu\n", (unsigned long long)count[0], (unsigned long long)count[1],
           (unsigned long long)count[2], (unsigned long long)count[3]);
    return 0;
}
