// digest_core.h on the CPU: the functions the kernels of ntcomp_amd/csrc/digest.hip call,
// walked the way k_dg_sum walks them -- the strings back to back in a buffer of aligned 64-bit
// words, each word of a string from one or two aligned loads, a funnel shift and the tail mask,
// the words dealt to 16 "lanes" (256 for a string past the long threshold) whose partial sums
// are added at the end -- so that ASan + UBSan see every load and the arithmetic.
// tests/test_digest.py builds it with -fsanitize=address,undefined and compares its output with
// digest_lib.py.
//
//   digest_cpu < IN > OUT
// IN (stdin):  u32 block_reads, u32 lead (bytes before the first string, so that strings start
//              at every misalignment), u64 n, then per string u32 bytes + the bytes
// OUT (stdout): one line "h <16 hex digits>" per string, then one line "D <16 hex digits>" per
//              block of block_reads strings
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../ntcomp_amd/csrc/digest_core.h"

using namespace ntc;

namespace {

constexpr uint64_t kLong = 2048;  // kernels.h kDgLong

// the buffer holds exactly the aligned words that cover the strings: a load past the word
// that holds a string's last byte is a heap overflow ASan reports
uint64_t load_word(const std::vector<uint64_t> &q, uint64_t p, uint64_t n, uint64_t j) {
    const uint32_t mis = (uint32_t)(p & 7);
    const uint64_t at = (p >> 3) + j;
    const uint64_t lo = q.at(at);
    const uint64_t hi = dg_needs_hi(n, j, mis) ? q.at(at + 1) : 0;
    return dg_funnel(lo, hi, 8 * mis) & dg_tail_mask(n, j);
}

uint64_t h_walk(const std::vector<uint64_t> &q, uint64_t p, uint64_t n) {
    const uint32_t lanes = n > kLong ? 256 : 16;
    std::vector<uint64_t> part(lanes, 0);
    const uint64_t words = dg_words(n);
    for (uint32_t lane = 0; lane < lanes; lane++)
        for (uint64_t j = lane; j < words; j += lanes) part[lane] += dg_word_term(load_word(q, p, n, j), j);
    uint64_t inner = 0;
    for (uint64_t v : part) inner += v;
    return dg_string(n, inner);
}

}  // namespace

int main() {
    std::vector<uint8_t> in;
    uint8_t chunk[1 << 16];
    size_t got;
    while ((got = std::fread(chunk, 1, sizeof(chunk), stdin)) > 0) in.insert(in.end(), chunk, chunk + got);
    if (in.size() < 16) return 2;
    uint32_t block_reads, lead;
    uint64_t n;
    std::memcpy(&block_reads, in.data(), 4);
    std::memcpy(&lead, in.data() + 4, 4);
    std::memcpy(&n, in.data() + 8, 8);
    if (block_reads == 0) return 2;
    std::vector<uint8_t> bytes(lead, 0xEE);
    std::vector<uint64_t> start(n), len(n);
    size_t at = 16;
    for (uint64_t r = 0; r < n; r++) {
        uint32_t l;
        if (in.size() - at < 4) return 2;
        std::memcpy(&l, in.data() + at, 4);
        at += 4;
        if (in.size() - at < l) return 2;
        start[r] = bytes.size();
        len[r] = l;
        bytes.insert(bytes.end(), in.begin() + at, in.begin() + at + l);
        at += l;
    }
    std::vector<uint64_t> q((bytes.size() + 7) / 8, 0);
    // what lies past the last string in its word is not zero: the tail mask must hide it
    std::memset(q.data(), 0xEE, q.size() * 8);
    if (!bytes.empty()) std::memcpy(q.data(), bytes.data(), bytes.size());
    std::vector<uint64_t> hs(n);
    for (uint64_t r = 0; r < n; r++) {
        hs[r] = h_walk(q, start[r], len[r]);
        std::printf("h %016llx\n", (unsigned long long)hs[r]);
    }
    for (uint64_t r0 = 0; r0 < n; r0 += block_reads) {
        uint64_t d = 0;
        for (uint64_t r = r0; r < n && r < r0 + block_reads; r++) d += dg_read_term(hs[r], r - r0);
        std::printf("D %016llx\n", (unsigned long long)d);
    }
    return 0;
}
