// TEST-ONLY stand-alone program (tests/test_parse_stage.py builds it with the address and
// undefined-behaviour sanitizers and runs it): k_parse4's staged query reader on the CPU.
//   parse_stage_cpu INDEX BLOCK[,BLOCK...] BATCH...
//   INDEX = {n, k, C[4]} as u64, 4 rows of ceil(n / 64) u64, n bytes of LCS
//   BATCH = {n_reads} as u64, n_reads + 1 read offsets as u64 (absolute, offs[0] may be > 0),
//           then offs[n_reads] bytes of bases
//   BLOCK = reads per block (k_parse4: 256); every batch is run with every block size
// The batch is packed into the 2-bit stream as k_pack lays it out (character x of the batch in
// word x / 32), every read's entries come from MsLaneT as in the emulator, and then each block of
// BLOCK reads is parsed twice: through the plain reader (the stream's pointer) and through a
// QStaged reader whose buffer is a heap block of exactly stage_word_count words copied from the
// stream at stage_first_word.  A query access outside the claimed range is then a heap overflow
// the sanitizer reports; the two parses must return the same records.  Prints
// "staged: R reads, B blocks, W words, N records" per batch and block size and returns 0, or says
// what differs.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../ntcomp_amd/csrc/derived.h"

using namespace ntc;

namespace {
bool read_all(FILE *f, void *p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

struct ReadState {  // what k_ms4 leaves for the parse of one read
    std::vector<Entry> Ed, Es, Ep;
    uint32_t ne = 0, obase = 0;
};

int fail(const char *what, uint64_t r) {
    printf("FAIL %s at read %llu\n", what, (unsigned long long)r);
    return 1;
}

// parse of one read through the reader Q; records to out (dense slots, then the pool)
template <class QR>
int parse_with(const DevIndex &d, const QR &Q, uint64_t P, uint32_t len, const ReadState &st, uint32_t S,
               std::vector<uint64_t> &out) {
    std::vector<uint64_t> R2(kRecSlot), Rp(len + 8);
    unsigned long long rcnt = 0, status = ~0ull;
    uint32_t rbase = 0;
    Entry pre[kEntSlot];
    for (uint32_t j = 0; j < kEntSlot; j++) pre[j] = st.Ed[j];
    const Entry *E1 = st.Es.data() - kEntSlot;
    const Entry *E2 = st.ne > kEntSlot + S ? st.Ep.data() + st.obase - kEntSlot - S : nullptr;
    const RecPool rp{Rp.data(), Rp.size(), &rcnt, &rbase, &status, 0};
    const int rc = parse_read(d, Q, P, E1, st.ne, len, R2.data(), nullptr, 1, st.Ed.data(), 1, pre, E2, S, &rp);
    out.clear();
    if (rc < 0 || status != ~0ull) return rc < 0 ? rc : -kErrCapacity;
    for (int j = 0; j < rc; j++) out.push_back(j < (int)kRecSlot ? R2[j] : Rp[rbase + j - kRecSlot]);
    return rc;
}
int run_batch(const DevIndex &d, const char *path, const std::vector<uint64_t> &block_sizes);
}  // namespace

int main(int argc, char **argv) {
    if (argc < 4) return 2;
    std::vector<uint64_t> block_sizes;
    for (const char *p = argv[2]; *p;) {
        char *end;
        block_sizes.push_back(strtoull(p, &end, 10));
        if (end == p || block_sizes.back() == 0) return 2;
        p = *end == ',' ? end + 1 : end;
    }
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

    // the index as the upload builds it for one genome (the emulator's load, its defaults with
    // NTC_EMU_JOINT=0: no joint runs, window and pair words, no filter)
    Derived dv;
    std::string err;
    if (!build_derived(hx, dv, err, true)) {
        printf("FAIL build_derived: %s\n", err.c_str());
        return 1;
    }
    std::vector<WalkEntry> walk;
    build_walk_host(dv, hx.n, walk);
    DevIndex d = host_dev_index(hx, dv, walk);
    d.rank2 = nullptr;
    d.joint = 0;
    const uint32_t U = default_tab_u(hx.n, hx.k, hx.lcs.data());
    d.tab_u = U;
    d.tab_pos = (dv.has_paths && U >= dv.t_jump && hx.n < (1ULL << 31)) ? 1u : 0u;
    std::vector<uint2> tab;
    std::vector<uint32_t> bits, fbits, winb;
    std::vector<uint16_t> pairb;
    build_tab_host(d, U, tab, bits, fbits);
    d.tab = tab.data();
    d.tab_bits = bits.data();
    d.filt_f = 0;
    d.filt_bits = nullptr;
    d.tab_u = U;
    d.win_w = nullptr;
    if (U >= 4) {
        winb.resize(win_words_count(U) * 8);
        for (uint64_t w = 0; w < winb.size(); w++) winb[w] = win_word(bits.data(), U, w >> 3, (uint32_t)(w & 7));
        d.win_w = winb.data();
    }
    pairb.resize(pair_words_count(U));
    for (uint64_t M = 0; M < pairb.size(); M++) pairb[M] = (uint16_t)pair_word(tab.data() + tab_base(U), U, M);
    d.pair_w = pairb.data();
    for (int i = 3; i < argc; i++) {
        const int rc = run_batch(d, argv[i], block_sizes);
        if (rc) return rc;
    }
    return 0;
}

namespace {
int run_batch(const DevIndex &d, const char *path, const std::vector<uint64_t> &block_sizes) {
    FILE *f = fopen(path, "rb");
    if (!f) return 2;
    uint64_t n_reads = 0;
    if (!read_all(f, &n_reads, 8)) return 2;
    std::vector<uint64_t> offs(n_reads + 1);
    if (!read_all(f, offs.data(), offs.size() * 8)) return 2;
    std::vector<uint8_t> bases(offs[n_reads]);
    if (!read_all(f, bases.data(), bases.size())) return 2;
    fclose(f);
    const uint64_t total = offs[n_reads] - offs[0];

    // k_pack: the stream, sized as capi.cpp sizes it
    std::vector<uint64_t> Q(total / 32 + 4, 0);
    for (uint64_t x = 0; x < total; x++) {
        const int c = base_code(bases[offs[0] + x]);
        if (c < 0) return fail("base", x);
        Q[x >> 5] |= (uint64_t)c << (2 * (x & 31));
    }

    // k_ms4, one read at a time
    const uint32_t S = 4;
    std::vector<ReadState> rs(n_reads);
    std::vector<uint4> stage((kStageSlots + 1) * 256);
    for (uint64_t r = 0; r < n_reads; r++) {
        const uint64_t P = offs[r] - offs[0];
        const uint32_t len = (uint32_t)(offs[r + 1] - offs[r]);
        if (len == 0) return fail("empty read", r);
        ReadState &st = rs[r];
        st.Ed.assign(kEntSlot, Entry{0, 0, 0, 0});
        st.Es.assign(S, Entry{0, 0, 0, 0});
        st.Ep.assign(len + 8, Entry{0, 0, 0, 0});
        unsigned long long pcnt = 0, status = ~0ull;
        const MsBufs bufs{Q.data(), st.Es.data(), st.Ed.data(), 1, stage.data(), kEntSlot, S, st.Ep.data(),
                          st.Ep.size(), &pcnt, &st.obase, &status};
        MsLaneT<false> ms;
        ms.start(d, P, len, 0, Q.data());
        for (;;) {
            const int rc = ms.step(d, bufs);
            if (rc < 0) return fail("matching statistics", r);
            if (rc == 1) break;
        }
        ms.finish(bufs);
        if (status != ~0ull) return fail("entry pool", r);
        st.ne = ms.ne;
        const uint32_t c0 = entry0_count(st.Ed[0]);
        if ((c0 == kNeInE0 ? st.ne : c0) != st.ne) return fail("entry count", r);
    }

    // k_parse4, block by block
    for (const uint64_t block : block_sizes) {
    uint64_t blocks = 0, words = 0, records = 0;
    std::vector<uint64_t> plain, staged;
    for (uint64_t r0 = 0; r0 < n_reads; r0 += block) {
        const uint64_t r1 = r0 + block < n_reads ? r0 + block : n_reads;
        const uint64_t b = offs[r0] - offs[0], e = offs[r1] - offs[0];
        const uint64_t w0 = stage_first_word(b), n = stage_word_count(b, e);
        if (w0 + n > Q.size()) return fail("stage past the stream's allocation", r0);
        uint64_t *buf = (uint64_t *)malloc(n * 8);  // exactly the claimed words
        if (!buf) return 2;
        memcpy(buf, Q.data() + w0, n * 8);
        const QStaged<const uint64_t *> reader{buf, w0};
        for (uint64_t r = r0; r < r1; r++) {
            const uint64_t P = offs[r] - offs[0];
            const uint32_t len = (uint32_t)(offs[r + 1] - offs[r]);
            const int a = parse_with(d, (const uint64_t *)Q.data(), P, len, rs[r], S, plain);
            const int s = parse_with(d, reader, P, len, rs[r], S, staged);
            if (a <= 0) return fail("plain parse", r);
            if (s != a || staged != plain) return fail("staged parse differs", r);
            records += (uint64_t)a;
        }
        free(buf);
        blocks++;
        words += n;
    }
    printf("staged: %llu reads, %llu blocks, %llu words, %llu records\n", (unsigned long long)n_reads,
           (unsigned long long)blocks, (unsigned long long)words, (unsigned long long)records);
    }
    return 0;
}
}  // namespace
