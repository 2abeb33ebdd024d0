// BGZF members of a text in HBM (`decode --bgzf`, ntc_bgzf_compress; bgzf_core.h has the plan's
// rule, deflate_core.h the coder, DESIGN.md §28 the design):
//   k_bgzf_plan    one workgroup.  A lane per grid point finds its cut by binary search in the
//                  record offsets; a lane per cell counts the cell's members and chunks, and a
//                  block scan per tile of 256 cells, with the tiles' carry, gives each cell its
//                  first member and chunk.  Then a lane per member finds its cell by binary
//                  search in those and writes the member's and its chunks' descriptors.
//                  counts[0..2] = members, chunks, text bytes.
//   k_bgzf_chunks  workgroups of one wave take chunks in a grid-stride loop: df_code_chunk with
//                  64 lanes, the chunk and its tables in LDS (DfWork).  The tokens pass through
//                  the workgroup's own 128 KiB of global memory, the bytes go to the chunk's slot.
//   k_bgzf_layout  one workgroup.  A lane per member adds up its size and joins its chunks'
//                  CRC-32; the same tiled block scan places the members back to back; a lane per
//                  member writes header, BSIZE and trailer and tells each chunk its place.
//                  counts[3] = bytes, counts[4..6] = chunks stored / Huffman / Huffman with matches.
//   then deflate.hip's k_df_place copies every chunk from its slot to its place.
// The host reads counts[0..2] between the plan and the coder and launches exact grids.
#include <hip/hip_runtime.h>

#include "bgzf_core.h"
#include "kernels.h"

namespace ntc {

namespace {

constexpr uint32_t kT = 256;  // lanes of the plan and layout workgroups, and cells / members per scan tile

static_assert(sizeof(DfWork) <= 80 * 1024, "two workgroups of k_bgzf_chunks share a CU's 160 KB of LDS");

// exclusive scan of v over the workgroup's kT lanes; *total = the sum (sh: kT words)
__device__ __forceinline__ uint64_t block_scan_excl(uint64_t v, uint64_t *sh, uint64_t *total) {
    const uint32_t t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (uint32_t d = 1; d < kT; d <<= 1) {
        const uint64_t x = t >= d ? sh[t - d] : 0;
        __syncthreads();
        sh[t] += x;
        __syncthreads();
    }
    const uint64_t incl = sh[t];
    *total = sh[kT - 1];
    __syncthreads();
    return incl - v;
}

__global__ __launch_bounds__(kT) void k_bgzf_plan(BgzfArgs a) {
    __shared__ uint64_t sh[kT];
    const uint32_t t = threadIdx.x;
    // the cuts, one lane per grid point
    for (uint64_t j = t; j <= a.n_cells; j += kT) a.cuts[j] = bgzf_cut(a.off, a.n_rec, a.off_base, a.n, j);
    __syncthreads();
    // members and chunks per cell, scanned
    uint64_t carry = 0;
    for (uint64_t j0 = 0; j0 < a.n_cells; j0 += kT) {
        const uint64_t j = j0 + t;
        const uint64_t v = j < a.n_cells ? bgzf_cell_counts(a.cuts[j + 1] - a.cuts[j]) : 0;
        uint64_t total;
        const uint64_t ex = block_scan_excl(v, sh, &total);
        if (j < a.n_cells) a.cell_first[j] = carry + ex;
        carry += total;
    }
    if (t == 0) {
        a.cell_first[a.n_cells] = carry;
        a.counts[0] = carry >> 32;
        a.counts[1] = carry & 0xFFFFFFFFu;
        a.counts[2] = a.n;
    }
    __syncthreads();
    // the descriptors, one lane per member
    // (offsets that do not ascend could count past the tables: the host refuses those counts)
    const uint64_t n_members = (carry >> 32) <= a.max_members && (carry & 0xFFFFFFFFu) <= a.max_chunks ? carry >> 32 : 0;
    for (uint64_t m = t; m < n_members; m += kT) {
        uint64_t lo = 0, hi = a.n_cells - 1;  // the last cell whose first member is <= m: the one that holds it
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo + 1) / 2;
            if ((a.cell_first[mid] >> 32) <= m)
                lo = mid;
            else
                hi = mid - 1;
        }
        const uint64_t first = a.cell_first[lo];
        uint64_t start, chunk0;
        uint32_t len;
        bgzf_member_at(a.cuts[lo], a.cuts[lo + 1], m - (first >> 32), first & 0xFFFFFFFFu, &start, &len, &chunk0);
        a.members[m] = BgzfMember{start, len, 0, 0};
        a.member_chunk[m] = (uint32_t)chunk0;
        for (uint32_t c = 0; c < bgzf_chunks_of(len); c++) {
            DfChunkDesc d;
            bgzf_chunk_at(start, len, c, &d.src_off, &d.n, &d.last);
            a.chunks[chunk0 + c] = d;
        }
    }
}

__global__ __launch_bounds__(64) void k_bgzf_chunks(const uint8_t *text, const DfChunkDesc *chunks, uint32_t n_chunks,
                                                    uint32_t *all_tokens, uint8_t *stage, DfResult *results) {
    __shared__ DfWork W;
    uint32_t *tokens = all_tokens + (uint64_t)blockIdx.x * kDfChunk;
    for (uint32_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const DfChunkDesc d = chunks[c];
        df_code_chunk(&W, text + d.src_off, d.n, d.last != 0, tokens, stage + (uint64_t)c * kDfSlot, results + c, threadIdx.x, 64);
        __syncthreads();  // (a lane still copying a stored chunk out of W.data: the next chunk overwrites it)
    }
}

__global__ __launch_bounds__(kT) void k_bgzf_layout(BgzfArgs a) {
    __shared__ uint64_t sh[kT];
    __shared__ uint32_t choices[4];
    const uint32_t t = threadIdx.x;
    if (t < 4) choices[t] = 0;
    __syncthreads();
    const uint32_t x_full = df_gf_xpow8(kDfChunk);
    // sizes and checksums
    for (uint64_t m = t; m < a.n_members; m += kT) {
        const uint32_t len = (uint32_t)a.members[m].text_bytes, c0 = a.member_chunk[m];
        uint32_t body = 0, crc = 0;
        for (uint32_t i = 0; i < bgzf_chunks_of(len); i++) {
            const DfResult r = a.results[c0 + i];
            const uint32_t n = a.chunks[c0 + i].n;
            body += r.size;
            crc = i ? df_crc_join(crc, r.crc, n == kDfChunk ? x_full : df_gf_xpow8(n)) : r.crc;
            atomicAdd(&choices[r.choice & 3], 1u);
        }
        a.members[m].bytes = kBgzfHeader + body + kBgzfTrailer;
        a.crcs[m] = crc;
    }
    __syncthreads();
    // places
    uint64_t carry = 0;
    for (uint64_t m0 = 0; m0 < a.n_members; m0 += kT) {
        const uint64_t m = m0 + t;
        uint64_t total;
        const uint64_t ex = block_scan_excl(m < a.n_members ? a.members[m].bytes : 0, sh, &total);
        if (m < a.n_members) a.members[m].place = carry + ex;
        carry += total;
    }
    if (t == 0) {
        a.counts[3] = carry;
        for (uint32_t i = 1; i < 4; i++) a.counts[3 + i] = choices[i];
    }
    __syncthreads();
    // headers, trailers, the chunks' places
    for (uint64_t m = t; m < a.n_members; m += kT) {
        const BgzfMember mb = a.members[m];
        const uint32_t c0 = a.member_chunk[m];
        uint64_t pos = mb.place + kBgzfHeader;
        for (uint32_t i = 0; i < bgzf_chunks_of((uint32_t)mb.text_bytes); i++) {
            a.chunk_off[c0 + i] = pos;
            pos += a.results[c0 + i].size;
        }
        bgzf_frame(a.out + mb.place, (uint32_t)(mb.bytes - kBgzfHeader - kBgzfTrailer), a.crcs[m], (uint32_t)mb.text_bytes);
    }
}

}  // namespace

void launch_bgzf_plan(const BgzfArgs &a, hipStream_t s) { hipLaunchKernelGGL(k_bgzf_plan, dim3(1), dim3(kT), 0, s, a); }

void launch_bgzf_code(const BgzfArgs &a, hipStream_t s) {
    if (a.n_members == 0) return;
    hipLaunchKernelGGL(k_bgzf_chunks, dim3(a.n_chunks < a.workgroups ? a.n_chunks : a.workgroups), dim3(64), 0, s, a.text,
                       (const DfChunkDesc *)a.chunks, a.n_chunks, a.tokens, a.stage, a.results);
    hipLaunchKernelGGL(k_bgzf_layout, dim3(1), dim3(kT), 0, s, a);
    DfArgs p{};
    p.n_chunks = a.n_chunks;
    p.stage = a.stage;
    p.results = a.results;
    p.chunk_off = a.chunk_off;
    p.out = a.out;
    launch_deflate_place(p, s);
}

}  // namespace ntc
