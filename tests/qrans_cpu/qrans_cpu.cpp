// The per-row and per-lane logic of qrans.hip on the CPU: the very functions of qrans_core.h,
// driven as the kernels drive them (counts per (context, symbol), a row per thread, a span per
// lane that writes backward from the end of its scratch slot, a lane per span that decodes
// with clamped reads), built under ASan + UBSan by tests/test_qrans.py.
//
//   qrans_cpu IN OUT
// IN : u32 n_syms, u32 0, u64 n_quals, then n_quals symbols (a byte each, < n_syms)
// OUT: the section body (table, span sizes, span streams); the test compares it with the
//      checker's (tests/qrans_lib.py) byte for byte.
// Asserted here: every adjusted frequency of a non-empty row is >= 1 and the row sums to 4096;
// no span is longer than qr_span_bound; the body passes qr_body_ok; the body decodes back to
// the symbols with every check of the decoder clear.
#include <cassert>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../ntcomp_amd/csrc/qrans_core.h"

using namespace ntc;

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                 \
        }                                                                 \
    } while (0)

static std::vector<uint8_t> read_file(const char *p) {
    FILE *f = std::fopen(p, "rb");
    CHECK(f);
    std::vector<uint8_t> b;
    uint8_t chunk[1 << 16];
    size_t got;
    while ((got = std::fread(chunk, 1, sizeof(chunk), f)) > 0) b.insert(b.end(), chunk, chunk + got);
    std::fclose(f);
    return b;
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    const std::vector<uint8_t> in = read_file(argv[1]);
    CHECK(in.size() >= 16);
    uint32_t n;
    uint64_t nq;
    std::memcpy(&n, in.data(), 4);
    std::memcpy(&nq, in.data() + 8, 8);
    CHECK(n <= kQRMaxSyms && in.size() == 16 + nq);
    const uint8_t *sym = in.data() + 16;
    std::vector<uint8_t> body;
    if (n > 1) {
        // k_qr_hist
        std::vector<uint32_t> cnt((n + 1) * n, 0);
        for (uint64_t i = 0; i < nq; i++) {
            CHECK(sym[i] < n);
            const uint32_t ctx = i % kQRSpan ? sym[i - 1] : n;
            cnt[ctx * n + sym[i]]++;
        }
        // k_qr_norm: a cumulative row per context
        std::vector<uint16_t> cum((n + 1) * kQRRow, 0);
        for (uint32_t r = 0; r <= n; r++) {
            uint16_t *row = cum.data() + r * kQRRow;
            qr_normalise(cnt.data() + r * n, n, row + 1);
            uint64_t total = 0;
            uint32_t sum = 0;
            for (uint32_t s = 0; s < n; s++) {
                total += cnt[r * n + s];
                sum += row[s + 1];
                CHECK((row[s + 1] >= 1) == (cnt[r * n + s] > 0));  // the adjusted one too
                CHECK(row[s + 1] <= kQRTotal);
            }
            CHECK(sum == (total ? kQRTotal : 0));
            row[0] = 0;
            uint32_t acc = 0;
            for (uint32_t s = 0; s < n; s++) {
                acc += row[s + 1];
                row[s + 1] = (uint16_t)acc;
            }
        }
        // k_qr_encode: backward from the end of a slot, a 32-bit word per store
        const uint64_t ns = qr_spans(nq);
        std::vector<std::vector<uint8_t>> streams(ns);
        for (uint64_t j = 0; j < ns; j++) {
            const uint32_t n_in = (uint32_t)(nq - j * kQRSpan < kQRSpan ? nq - j * kQRSpan : kQRSpan);
            const uint8_t *src = sym + j * kQRSpan;
            std::vector<uint8_t> slot(qr_span_bound(kQRSpan) + 4);  // (+ 4: the last word store may start below the stream)
            uint8_t *const end = slot.data() + slot.size(), *p = end;
            uint32_t x = kQRL, acc = 0, na = 0;
            const auto emit = [&](uint32_t byte) {
                acc = acc << 8 | byte;
                if (++na == 4) {
                    p -= 4;
                    CHECK(p >= slot.data());
                    std::memcpy(p, &acc, 4);
                    na = 0;
                }
            };
            for (uint32_t i = n_in; i-- > 0;) {
                const uint32_t ctx = i ? src[i - 1] : n;
                const uint16_t *row = cum.data() + ctx * kQRRow;
                const uint32_t cs = row[src[i]], f = row[src[i] + 1] - cs;
                CHECK(f >= 1 && x >= kQRL && x < (1u << 31));
                x = qr_encode_step(x, cs, f, emit);
            }
            CHECK(x >= kQRL && x < (1u << 31));
            emit(x >> 24);
            emit((x >> 16) & 0xFF);
            emit((x >> 8) & 0xFF);
            emit(x & 0xFF);
            for (uint32_t t = na; t-- > 0;) *--p = (uint8_t)(acc >> (8 * t));
            streams[j].assign(p, end);
            CHECK(streams[j].size() <= qr_span_bound(n_in));  // the slot-stride bound
        }
        // k_qr_place
        for (uint32_t r = 0; r <= n; r++)
            for (uint32_t s = 0; s < n; s++) {
                const uint16_t f = (uint16_t)(cum[r * kQRRow + s + 1] - cum[r * kQRRow + s]);
                body.push_back((uint8_t)(f & 0xFF));
                body.push_back((uint8_t)(f >> 8));
            }
        for (uint64_t j = 0; j < ns; j++) {
            const uint32_t size = (uint32_t)streams[j].size();
            for (int t = 0; t < 4; t++) body.push_back((uint8_t)(size >> (8 * t)));
        }
        for (uint64_t j = 0; j < ns; j++) body.insert(body.end(), streams[j].begin(), streams[j].end());
        CHECK(qr_body_ok(nq, n, body.data(), body.size()));
        // k_qr_decode, from the body alone
        std::vector<uint16_t> tab((n + 1) * kQRRow, 0);
        for (uint32_t r = 0; r <= n; r++) {
            uint32_t acc = 0;
            for (uint32_t c = 0; c < n; c++) {
                acc += body[2 * (r * n + c)] | body[2 * (r * n + c) + 1] << 8;
                tab[r * kQRRow + c + 1] = (uint16_t)acc;
            }
        }
        uint64_t pos = qr_table_bytes(n) + 4 * ns;
        for (uint64_t j = 0; j < ns; j++) {
            const uint32_t n_in = (uint32_t)(nq - j * kQRSpan < kQRSpan ? nq - j * kQRSpan : kQRSpan);
            const uint64_t en = pos + streams[j].size();
            bool bad = false;
            const auto next = [&]() -> uint32_t {
                if (pos < en) return body[pos++];
                bad = true;
                return 0;
            };
            uint32_t x = next();
            x |= next() << 8;
            x |= next() << 16;
            x |= next() << 24;
            uint32_t ctx = n;
            for (uint32_t i = 0; i < n_in; i++) {
                const uint16_t *row = tab.data() + ctx * kQRRow;
                const uint32_t slot = x & (kQRTotal - 1);
                CHECK(slot < row[n]);
                const uint32_t s = qr_find(row, n, slot);
                CHECK(s == sym[j * kQRSpan + i]);
                x = qr_decode_step(x, row[s], row[s + 1] - row[s]);
                CHECK(x >= (1u << 11));  // two bytes refill it
                CHECK(qr_refill(x, next));
                ctx = s;
            }
            CHECK(!bad && x == kQRL && pos == en);
        }
    } else {
        CHECK(qr_body_ok(nq, n, nullptr, 0));
    }
    FILE *f = std::fopen(argv[2], "wb");
    CHECK(f);
    if (!body.empty()) CHECK(std::fwrite(body.data(), 1, body.size(), f) == body.size());
    CHECK(std::fclose(f) == 0);
    return 0;
}
