// A window on a decoded batch's text: the rule of window.hip and of the formatters' windowed
// writers (fasta.hip, quality.hip, names.hip, pairs.hip).  Written once as host + device code,
// like pair_core.h: the HIP kernels call these functions, and a CPU program (tests/window_cpu)
// compiles the very same functions with a host compiler, so the rule is tested without a GPU.
//
// Vocabulary (DESIGN.md "Decoding a range"): a batch of n reads is decoded whole -- walk,
// exception patch, qualities, names, digests -- and only reads [first, first + count) of it are
// formatted.  Read r keeps what it has in the whole batch: the id first_id + r, its name, its
// quality line.  The formatters size every read, the window zeroes the sizes outside it before
// the exclusive scan, and a writer skips a read whose record is empty (no record of a format
// here is: the shortest, ">\n\n", has three bytes).
#pragma once
#include <cstdint>

#include "names_core.h"

namespace ntc {

// the request: count >= 1 reads inside the batch; whole pairs under the "paired" option
N_HD bool w_valid(uint64_t first, uint64_t count, uint64_t n_reads, bool paired) {
    if (count == 0 || first >= n_reads || count > n_reads - first) return false;
    return !paired || ((first | count) & 1) == 0;
}

// read r of the batch is formatted
N_HD bool w_keeps(uint64_t r, uint64_t first, uint64_t count) { return r >= first && r - first < count; }

// its record's bytes, given the bytes it has in the whole batch's text
N_HD uint64_t w_size(uint64_t size, uint64_t r, uint64_t first, uint64_t count) {
    return w_keeps(r, first, count) ? size : 0;
}

// a writer's test, from the scanned offsets of the read and of the next one
N_HD bool w_skips(uint64_t off, uint64_t off_next) { return off_next == off; }

}  // namespace ntc
