// pair_core.h on the CPU: the weave's text checks, record spans and places, the mate rule in
// the kernels' 64-byte ballot steps, and the split's places, over a case tests/test_pairs.py
// writes.  Built by the test under ASan + UBSan; compared there against tests/pair_lib.py.
//
// in:  u64 n_pairs, u64 bytes1, text1, u64 bytes2, text2
// out: u64 weave status (~0, or read << 8 | 8), u64 check status (~0, or (2 p) << 8 | 8),
//      u64 woven bytes, the woven text, u64 bytes of part 1, the split text (woven bytes)
//      (nothing after the weave status when it is set)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "../../ntcomp_amd/csrc/pair_core.h"

using namespace ntc;

namespace {

constexpr uint64_t kOk = ~0ull, kFormat = 8;

struct Text {
    std::vector<uint8_t> raw;
    std::vector<uint32_t> nl;  // the first nl_cap newlines, as k_fq_lines leaves them
    uint64_t n_nl = 0;
    uint32_t last() const { return raw.empty() ? 0 : raw.back(); }
};

void lines(Text &t, uint64_t nl_cap) {
    for (uint64_t i = 0; i < t.raw.size(); i++) {
        if (t.raw[i] != '\n') continue;
        if (t.n_nl < nl_cap) t.nl.push_back((uint32_t)i);
        t.n_nl++;
    }
}

// a wave's ballot over 64 lanes
template <class F>
uint64_t ballot(F f) {
    uint64_t m = 0;
    for (uint32_t lane = 0; lane < 64; lane++) m |= (uint64_t)(f(lane) ? 1 : 0) << lane;
    return m;
}

struct Name {
    uint64_t s;
    uint32_t len;
};
Name id_of(const Text &t, uint64_t r) {  // pairs.hip p_id
    const uint64_t h0 = r ? (uint64_t)t.nl[4 * r - 1] + 1 : 0, e = t.nl[4 * r];
    Name f;
    f.s = h0 + 1 < e ? h0 + 1 : e;
    uint32_t len = (uint32_t)(e - f.s);
    if (len && t.raw[e - 1] == '\r') len--;
    for (uint32_t b = 0; b < len; b += 64) {
        const uint64_t m = ballot([&](uint32_t lane) { return b + lane < len && n_is_cut(t.raw[f.s + b + lane]); });
        if (p_cut_step(m, b, &len)) break;
    }
    f.len = len;
    return f;
}

bool agree(const Text &t, uint64_t p) {  // pairs.hip k_pm_check
    Name x = id_of(t, 2 * p), y = id_of(t, 2 * p + 1);
    if (p_strips(x.len, y.len, x.len >= 2 ? t.raw[x.s + x.len - 2] : 0, x.len >= 2 ? t.raw[x.s + x.len - 1] : 0,
                 y.len >= 2 ? t.raw[y.s + y.len - 2] : 0, y.len >= 2 ? t.raw[y.s + y.len - 1] : 0)) {
        x.len -= 2;
        y.len -= 2;
    }
    bool ok = x.len == y.len;
    for (uint32_t b = 0; ok && b < x.len; b += 64) {
        const uint64_t eq = ballot([&](uint32_t lane) { return b + lane < x.len && t.raw[x.s + b + lane] == t.raw[y.s + b + lane]; });
        ok = p_step_agrees(eq, x.len, b);
    }
    return ok;
}

void put(std::vector<uint8_t> &o, uint64_t v) {
    for (int i = 0; i < 8; i++) o.push_back((uint8_t)(v >> (8 * i)));
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    std::vector<uint8_t> in((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    uint64_t at = 0, n_pairs = 0;
    const auto u64 = [&]() {
        uint64_t v = 0;
        std::memcpy(&v, in.data() + at, 8);
        at += 8;
        return v;
    };
    n_pairs = u64();
    Text t[2];
    for (int i = 0; i < 2; i++) {
        const uint64_t n = u64();
        t[i].raw.assign(in.begin() + at, in.begin() + at + n);
        at += n;
        lines(t[i], 4 * n_pairs);
    }
    std::vector<uint8_t> out;
    // k_pw_sizes
    bool ok[2];
    for (int i = 0; i < 2; i++) ok[i] = p_text_ok(t[i].n_nl, t[i].raw.size(), t[i].last(), n_pairs);
    if (!ok[0] || !ok[1]) {
        const int b = ok[0] ? 1 : 0;
        const uint64_t whole = p_lines(t[b].n_nl, t[b].raw.size(), t[b].last()) / 4;
        const uint64_t p = whole < n_pairs ? whole : (n_pairs ? n_pairs - 1 : 0);
        put(out, (2 * p + b) << 8 | kFormat);
    } else {
        std::vector<uint64_t> offs(n_pairs + 1, 0);
        for (uint64_t p = 0; p < n_pairs; p++) {
            uint64_t sz = 0;
            for (int i = 0; i < 2; i++) {
                sz += p_rec_end(t[i].nl.data(), t[i].n_nl, t[i].raw.size(), p) - p_rec_begin(t[i].nl.data(), p);
                if (p == n_pairs - 1 && p_adds_nl(t[i].raw.size(), t[i].last())) sz++;
            }
            offs[p + 1] = offs[p] + sz;
        }
        // k_pw_copy
        Text w;
        w.raw.assign(offs[n_pairs], 0xEE);
        for (uint64_t p = 0; p < n_pairs; p++) {
            uint64_t d = offs[p];
            for (int i = 0; i < 2; i++) {
                const uint64_t b = p_rec_begin(t[i].nl.data(), p), e = p_rec_end(t[i].nl.data(), t[i].n_nl, t[i].raw.size(), p);
                for (uint64_t j = b; j < e; j++) w.raw.at(d++) = t[i].raw.at(j);
                if (p == n_pairs - 1 && p_adds_nl(t[i].raw.size(), t[i].last())) w.raw.at(d++) = '\n';
            }
            if (d != offs[p + 1]) return 3;
        }
        lines(w, 8 * n_pairs);
        if (w.n_nl != 8 * n_pairs) return 4;
        // k_pm_check
        uint64_t st = kOk;
        for (uint64_t p = 0; p < n_pairs; p++)
            if (!agree(w, p)) st = st < ((2 * p) << 8 | kFormat) ? st : ((2 * p) << 8 | kFormat);
        put(out, kOk);
        put(out, st);
        put(out, w.raw.size());
        out.insert(out.end(), w.raw.begin(), w.raw.end());
        // k_ps_sizes, the scans, k_ps_copy: over the records of the woven text
        std::vector<uint64_t> ro(2 * n_pairs + 1, 0), o1(n_pairs + 1, 0), o2(n_pairs + 1, 0);
        for (uint64_t r = 0; r < 2 * n_pairs; r++) ro[r + 1] = (uint64_t)w.nl[4 * r + 3] + 1;
        for (uint64_t p = 0; p < n_pairs; p++) {
            o1[p + 1] = o1[p] + (ro[2 * p + 1] - ro[2 * p]);
            o2[p + 1] = o2[p] + (ro[2 * p + 2] - ro[2 * p + 1]);
        }
        std::vector<uint8_t> sp(w.raw.size(), 0xEE);
        for (uint64_t r = 0; r < 2 * n_pairs; r++) {
            const uint64_t d = p_split_at(r, o1.data(), o2.data(), n_pairs);
            for (uint64_t j = ro[r]; j < ro[r + 1]; j++) sp.at(d + j - ro[r]) = w.raw.at(j);
        }
        put(out, o1[n_pairs]);
        out.insert(out.end(), sp.begin(), sp.end());
    }
    std::ofstream o(argv[2], std::ios::binary);
    o.write((const char *)out.data(), (std::streamsize)out.size());
    return o.good() ? 0 : 5;
}
