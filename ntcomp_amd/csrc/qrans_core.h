// FASTQ quality scores, the order-1 rANS coder: the per-row and per-symbol logic of the
// kernels in qrans.hip.  Written once as host + device code, like quality_core.h: the HIP
// kernels call these functions, and a CPU program (tests/qrans_cpu) compiles the very same
// functions with a host compiler, so normalisation, the coder steps, the symbol search and the
// size bound are checked without a GPU.
//
// Vocabulary (DESIGN.md "Quality scores, rANS"): a block's qualities are cut into spans of
// kQRSpan; a quality's symbol is its rank in the block's alphabet, its context the symbol
// before it in the span, n_syms at a span's start.  Row `context` of the block's table holds
// the n_syms frequencies, each row summing to kQRTotal = 2^12 (or all zero: a context that
// never occurs).  A cumulative row has n_syms + 1 entries: cum[s] = the frequencies below s.
#pragma once
#include <cstdint>

#include "quality_core.h"

namespace ntc {

constexpr uint32_t kQRSpan = 2048;        // qualities per span
constexpr uint32_t kQRBits = 12;          // probability bits
constexpr uint32_t kQRTotal = 1u << kQRBits;
constexpr uint32_t kQRL = 1u << 23;       // the state lives in [L, 256 L)
constexpr uint32_t kQRMaxSyms = 94;
constexpr uint32_t kQRRow = 96;           // entries of a cumulative row as the kernels keep it (>= 95)

Q_HD uint64_t qr_spans(uint64_t n_quals) { return (n_quals + kQRSpan - 1) / kQRSpan; }

// bytes of the table at the head of a section body
Q_HD uint64_t qr_table_bytes(uint32_t n_syms) { return n_syms <= 1 ? 0 : 2ull * (n_syms + 1) * n_syms; }

// The most bytes a span of n <= kQRSpan symbols can take, the 4-byte state included.  Before a
// step the state x lies in [2^23, 2^31).  The step shifts out k bytes, leaving y <= x / 256^k,
// and y >= 2^11 whenever k > 0 (the byte before left y' >= 2^19 f); then x' = (y / f) 2^12 +
// y % f + c <= 2^12 (y + 1) - 1, as c + f <= 2^12.  So x' < 2^12 (1 + 2^-11) x / 256^k, and
// over n symbols with K bytes in all, 2^23 <= x_n < 2^23 (2^12 (1 + 2^-11))^n / 256^K, that is
// 8 K < 12 n + n log2(1 + 2^-11) < 12 n + 1.45 for n <= 2048.  8 K is a multiple of 8 and 12 n
// of 4, so 8 K <= 12 n - (12 n mod 8): K <= floor(3 n / 2).
Q_HD constexpr uint32_t qr_span_bound(uint32_t n) { return n + n / 2 + 4; }

// One row: counts c[0 .. n) -> frequencies f[0 .. n).  0 where the count is 0, else
// max(1, floor(c 4096 / T)); the difference to 4096 (which may be negative) goes to the symbol
// with the largest count, lowest index on ties.  A row with T = 0 is all zeros.  With n <= 94
// the adjusted frequency stays >= 1 (DESIGN.md has the bound).
Q_HD void qr_normalise(const uint32_t *c, uint32_t n, uint16_t *f) {
    uint64_t total = 0;
    uint32_t best = 0;
    for (uint32_t s = 0; s < n; s++) {
        total += c[s];
        if (c[s] > c[best]) best = s;
    }
    if (total == 0) {
        for (uint32_t s = 0; s < n; s++) f[s] = 0;
        return;
    }
    int32_t sum = 0, f_best = 0;
    for (uint32_t s = 0; s < n; s++) {
        uint32_t v = 0;
        if (c[s]) {
            v = (uint32_t)((uint64_t)c[s] * kQRTotal / total);
            if (v < 1) v = 1;
        }
        if (s == best) f_best = (int32_t)v;
        f[s] = (uint16_t)v;
        sum += (int32_t)v;
    }
    f[best] = (uint16_t)(f_best + ((int32_t)kQRTotal - sum));
}

// Encode one symbol of start c and frequency f (>= 1): bytes leave through emit(byte), at most
// two of them (x < 2^31 and 2^19 f >= 2^19); returns the new state.
template <class Emit>
Q_HD uint32_t qr_encode_step(uint32_t x, uint32_t c, uint32_t f, Emit &&emit) {
    const uint32_t lim = f << 19;  // f = 4096: 2^31, above every state
    for (uint32_t t = 0; t < 2; t++) {
        if (x < lim) break;
        emit(x & 0xFF);
        x >>= 8;
    }
    return ((x / f) << kQRBits) + (x % f) + c;
}

// The symbol of a slot in a cumulative row of n >= 1 symbols: the last s with cum[s] <= slot.
// For slot < cum[n] that symbol has cum[s + 1] > slot, so a frequency >= 1.  Seven halvings
// cover n <= 128, whatever the row holds.
Q_HD uint32_t qr_find(const uint16_t *cum, uint32_t n, uint32_t slot) {
    uint32_t lo = 0, hi = n;
    for (uint32_t t = 0; t < 7; t++) {
        const uint32_t mid = (lo + hi) / 2;
        if (hi - lo > 1) {
            if (cum[mid] <= slot) lo = mid;
            else hi = mid;
        }
    }
    return lo;
}

// Decode step: the state after symbol (c, f) was taken from slot = x & 4095, before the refill
Q_HD uint32_t qr_decode_step(uint32_t x, uint32_t c, uint32_t f) {
    return f * (x >> kQRBits) + (x & (kQRTotal - 1)) - c;
}

// Refill: at most two bytes by construction (x >= 2^11 after a step of a sound stream);
// next() yields the next byte of the span.  Returns false when the state is still below L.
template <class Next>
Q_HD bool qr_refill(uint32_t &x, Next &&next) {
    for (uint32_t t = 0; t < 2; t++) {
        if (x >= kQRL) break;
        x = x << 8 | next();
    }
    return x >= kQRL;
}

// A section body as a decoder may trust it (host): the table's rows sum to 4096 or are all
// zero, the start row is not zero when there are qualities, the span sizes follow from
// n_quals, each is >= 4, and they sum to the rest of the body; n_syms <= 1 has no body.
inline bool qr_body_ok(uint64_t n_quals, uint32_t n_syms, const uint8_t *body, uint64_t bytes) {
    if (n_syms <= 1) return bytes == 0;
    const uint64_t tb = qr_table_bytes(n_syms), ns = qr_spans(n_quals);
    if (n_syms > kQRMaxSyms || bytes < tb || (bytes - tb) / 4 < ns) return false;
    for (uint32_t r = 0; r <= n_syms; r++) {
        uint32_t sum = 0;
        for (uint32_t s = 0; s < n_syms; s++) {
            const uint8_t *p = body + 2 * ((uint64_t)r * n_syms + s);
            sum += (uint32_t)p[0] | (uint32_t)p[1] << 8;
        }
        if (sum != kQRTotal && (sum != 0 || (r == n_syms && n_quals > 0))) return false;
    }
    uint64_t left = bytes - tb - 4 * ns;
    for (uint64_t j = 0; j < ns; j++) {
        const uint8_t *p = body + tb + 4 * j;
        const uint32_t size = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
        if (size < 4 || size > left) return false;
        left -= size;
    }
    return left == 0;
}

}  // namespace ntc
