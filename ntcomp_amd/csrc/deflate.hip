// Deflate of the packed block streams on the device (`--deflate gpu`; deflate_core.h has the
// coder, DESIGN.md §26 the rules).  Over the payload the packer left in HBM:
//   k_df_chunks   one workgroup of one wave per chunk, the chunk and its tables in LDS
//                 (DfWork): df_code_chunk, the function the host restatement runs with one lane.
//                 The chunk's bytes go to its slot of the staging buffer, its size, CRC-32 and
//                 encoding to results; the tokens of encoding 3 pass through the workgroup's
//                 own piece of global memory.
//   k_df_layout   one workgroup: per stream the member's size and CRC-32 (the chunks' joined,
//                 x^(8 len) mod P), then the members' places back to back, then per stream the
//                 10 header bytes, the place of each chunk and the trailer.
//   k_df_place    one workgroup per chunk: its bytes from the slot to their place.
// Nothing here depends on the order in which lanes or workgroups arrive: the LDS atomics of the
// coder are max, or and add over integers, and every output byte has one writer.
#include <hip/hip_runtime.h>

#include "deflate_core.h"
#include "kernels.h"

namespace ntc {

namespace {

static_assert(sizeof(DfWork) <= 80 * 1024, "two workgroups of k_df_chunks share a CU's 160 KB of LDS");

__global__ __launch_bounds__(64) void k_df_chunks(DfArgs a) {
    __shared__ DfWork W;
    const uint32_t c = blockIdx.x;
    const DfChunkDesc d = a.chunks[c];
    df_code_chunk(&W, a.payload + d.src_off, d.n, d.last != 0, a.tokens + (uint64_t)c * kDfChunk,
                  a.stage + (uint64_t)c * kDfSlot, a.results + c, threadIdx.x, 64);
}

__global__ __launch_bounds__(256) void k_df_layout(DfArgs a) {
    // the members' sizes and checksums
    for (uint32_t s = threadIdx.x; s < a.n_streams; s += 256) {
        const DfStreamDesc st = a.streams[s];
        uint64_t len = 18;
        uint32_t crc = 0;
        const uint32_t x_full = df_gf_xpow8(kDfChunk);
        for (uint32_t i = 0; i < st.n_chunks; i++) {
            const uint32_t c = st.first_chunk + i, m = a.chunks[c].n;
            len += a.results[c].size;
            crc = i ? df_crc_join(crc, a.results[c].crc, m == kDfChunk ? x_full : df_gf_xpow8(m)) : a.results[c].crc;
        }
        a.member_off_len[2 * s + 1] = len;
        a.crcs[s] = crc;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t off = 0;
        for (uint32_t s = 0; s < a.n_streams; s++) {
            a.member_off_len[2 * s] = off;
            off += a.member_off_len[2 * s + 1];
        }
        a.member_off_len[2 * (uint64_t)a.n_streams] = off;
    }
    __syncthreads();
    for (uint32_t s = threadIdx.x; s < a.n_streams; s += 256) {
        const DfStreamDesc st = a.streams[s];
        uint8_t *o = a.out + a.member_off_len[2 * s];
        for (uint32_t i = 0; i < 10; i++) o[i] = df_gzip_header(i);
        uint64_t pos = a.member_off_len[2 * s] + 10;
        for (uint32_t i = 0; i < st.n_chunks; i++) {
            a.chunk_off[st.first_chunk + i] = pos;
            pos += a.results[st.first_chunk + i].size;
        }
        const uint32_t crc = a.crcs[s], isize = (uint32_t)st.n;
        for (uint32_t i = 0; i < 4; i++) a.out[pos + i] = (uint8_t)(crc >> (8 * i));
        for (uint32_t i = 0; i < 4; i++) a.out[pos + 4 + i] = (uint8_t)(isize >> (8 * i));
    }
}

__global__ __launch_bounds__(256) void k_df_place(DfArgs a) {
    const uint32_t c = blockIdx.x, size = a.results[c].size;
    const uint8_t *src = a.stage + (uint64_t)c * kDfSlot;
    uint8_t *dst = a.out + a.chunk_off[c];
    for (uint32_t i = threadIdx.x; i < size; i += 256) dst[i] = src[i];
}

}  // namespace

void launch_deflate(const DfArgs &a, hipStream_t s) {
    if (a.n_streams == 0) return;
    hipLaunchKernelGGL(k_df_chunks, dim3(a.n_chunks), dim3(64), 0, s, a);
    hipLaunchKernelGGL(k_df_layout, dim3(1), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_df_place, dim3(a.n_chunks), dim3(256), 0, s, a);
}

void launch_deflate_place(const DfArgs &a, hipStream_t s) {
    if (a.n_chunks == 0) return;
    hipLaunchKernelGGL(k_df_place, dim3(a.n_chunks), dim3(256), 0, s, a);
}

}  // namespace ntc
