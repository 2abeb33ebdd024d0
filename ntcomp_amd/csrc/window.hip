// A window on the text formatters (window_core.h): between a formatter's sizes kernel and its
// exclusive scan, the sizes of the reads outside [first, first + count) become 0, so the scan
// packs the window's records at the head of the text and the windowed writers skip the rest.
//   k_window_sizes  one thread per read outside the window: sizes[r] = 0.  The grid covers
//                   only the n - count reads outside (r < first, then r >= first + count), so
//                   a narrow window in a large batch costs one pass of stores and a wide one
//                   next to nothing; nothing is loaded.
//   k_window_box    the window's bytes (the scan's total) into the host's box, so that the
//                   call copies only them
// Neither runs for a call without a window.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "window_core.h"

namespace ntc {

namespace {

__global__ __launch_bounds__(256) void k_window_sizes(uint64_t *sizes, uint64_t n, uint64_t first, uint64_t count) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t r = t < first ? t : t + count;  // the t-th read outside the window
    if (r >= n) return;
    if (!w_keeps(r, first, count)) sizes[r] = 0;  // (always: r is outside by construction; the rule stays in one place)
}

__global__ void k_window_box(const uint64_t *total, uint64_t *box) { box[kBoxWindow] = *total; }

}  // namespace

void launch_window_sizes(uint64_t *sizes, uint64_t n, uint64_t first, uint64_t count, hipStream_t s) {
    const uint64_t outside = n - count;
    if (!outside) return;
    hipLaunchKernelGGL(k_window_sizes, dim3((uint32_t)((outside + 255) / 256)), dim3(256), 0, s, sizes, n, first, count);
}

void launch_window_box(const uint64_t *total, uint64_t *box, hipStream_t s) {
    hipLaunchKernelGGL(k_window_box, dim3(1), dim3(1), 0, s, total, box);
}

}  // namespace ntc
