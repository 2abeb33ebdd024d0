// Inflate of gzip members of at most 64 KiB on the device (`--inflate gpu`,
// ntc_inflate_members; inflate_core.h has the decoder, DESIGN.md §27 the rules):
//   k_inf_members  one workgroup of one wave per member, the member's output window and its
//                  tables in LDS (InfWork): inf_member, the function the host restatement runs
//                  with one lane.  A sound member's bytes go from the window straight to their
//                  place in dst, its status, size and CRC-32 to results; a member that fails
//                  writes its result alone.
// Nothing needs placing or compacting afterwards: the caller knows every member's place from
// its ISIZE before the launch.  Nothing here depends on the order in which lanes or workgroups
// arrive: the one LDS atomic of the decoder is an integer add, and every output byte has one
// writer.
#include <hip/hip_runtime.h>

#include "inflate_core.h"
#include "kernels.h"

namespace ntc {

namespace {

static_assert(sizeof(InfWork) <= 80 * 1024, "two workgroups of k_inf_members share a CU's 160 KB of LDS");

__global__ __launch_bounds__(64) void k_inf_members(InfArgs a) {
    __shared__ InfWork W;
    const InfMemberDesc m = a.members[blockIdx.x];
    inf_member(&W, a.comp + m.src_off, m.src_bytes, m.out_bytes, a.dst + m.dst_off, a.results + blockIdx.x, threadIdx.x, 64);
}

}  // namespace

void launch_inflate(const InfArgs &a, hipStream_t s) {
    if (a.n_members == 0) return;
    hipLaunchKernelGGL(k_inf_members, dim3(a.n_members), dim3(64), 0, s, a);
}

}  // namespace ntc
