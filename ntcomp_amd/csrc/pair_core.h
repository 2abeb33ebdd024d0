// Paired-end reads: the mate rule and the offset arithmetic of the kernels in pairs.hip.
// Written once as host + device code, like names_core.h: the HIP kernels call these
// functions, and a CPU program (tests/pair_cpu) compiles the very same functions with a host
// compiler and walks them in the kernels' 64-byte steps, so the rule, the record spans and the
// count checks are tested without a GPU.
//
// Vocabulary (DESIGN.md "Paired-end reads"): a paired archive alternates, read 2p is mate 1 of
// pair p and read 2p + 1 its mate 2.  id(N) is the name N cut before its first space or tab.
// With a = id(name1) and b = id(name2): when a ends in "/1" and b ends in "/2" both lose those
// two bytes; the mates agree iff a == b byte for byte.
#pragma once
#include <cstdint>

#include "names_core.h"

namespace ntc {

constexpr int kPairOff = 0, kPairIds = 1, kPairNoCheck = 2;  // the "paired" option

// ---- the weave's text checks and record spans ----------------------------------------------
// nl: the text's newline positions (the first 4 n of them at most), n_nl: newlines found in
// all, n_raw: the text's bytes, last: its last byte (any value when n_raw = 0).

// lines of a text: a trailing line without its newline counts as one
N_HD uint64_t p_lines(uint64_t n_nl, uint64_t n_raw, uint32_t last) {
    return n_nl + (n_raw != 0 && last != '\n' ? 1 : 0);
}
// the text is n whole four-line records
N_HD bool p_text_ok(uint64_t n_nl, uint64_t n_raw, uint32_t last, uint64_t n) { return p_lines(n_nl, n_raw, last) == 4 * n; }
// the weave adds a newline after the text's last line
N_HD bool p_adds_nl(uint64_t n_raw, uint32_t last) { return n_raw != 0 && last != '\n'; }

// record r of a text p_text_ok took: first byte, and the bytes to copy (its newlines included,
// the one the last line may lack not)
N_HD uint64_t p_rec_begin(const uint32_t *nl, uint64_t r) { return r ? (uint64_t)nl[4 * r - 1] + 1 : 0; }
N_HD uint64_t p_rec_end(const uint32_t *nl, uint64_t n_nl, uint64_t n_raw, uint64_t r) {
    return 4 * r + 3 < n_nl ? (uint64_t)nl[4 * r + 3] + 1 : n_raw;
}

// ---- the mate rule ------------------------------------------------------------------------
// One 64-byte step of the id cut: bit j of cut says that byte b + j of the name is a space or a
// tab (bits past the name's end are 0).  Returns true when the cut lies in this step and sets
// *len to it.
N_HD bool p_cut_step(uint64_t cut, uint32_t b, uint32_t *len) {
    if (!cut) return false;
    *len = b + n_ctz(cut);
    return true;
}

// the "/1" "/2" strip: t1 / t2 = the last two bytes of each id (only read when len >= 2)
N_HD bool p_strips(uint32_t len1, uint32_t len2, uint32_t t1a, uint32_t t1b, uint32_t t2a, uint32_t t2b) {
    return len1 >= 2 && len2 >= 2 && t1a == '/' && t1b == '1' && t2a == '/' && t2b == '2';
}

// One 64-byte step of the comparison, over ids of equal length len from byte b: n_run of the
// live lanes; the mates disagree when a live lane differs.
N_HD bool p_step_agrees(uint64_t eq, uint32_t len, uint32_t b) {
    const uint32_t live = len - b < 64 ? len - b : 64;
    return n_run(eq, live) == live;
}

// ---- the split's places --------------------------------------------------------------------
// read r of a paired decode goes to part r & 1 at the scanned offset of its pair; part 2
// starts where part 1 ends
N_HD uint64_t p_split_at(uint64_t r, const uint64_t *o1, const uint64_t *o2, uint64_t n_pairs) {
    return r & 1 ? o1[n_pairs] + o2[r >> 1] : o1[r >> 1];
}

}  // namespace ntc
