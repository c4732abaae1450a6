// Rows gathered from independent allocations: the stack behind consolidation.consolidate_short_term_memory
// (hippomm_amd/consolidation.py).  The reference stacks one 1024-float row per frame, picked out of every segment's own feature
// block, in time order (hippocampal_memory.py:842); here the blocks stay where they lie on the device and a table of row ADDRESSES
// says which 4 KB goes where.  Unlike store_gather_kernel (store_ingest.hip) there is no common source buffer and no segment
// table: every row is addressed by itself, any row any number of times, in any order.
//
//   one wave64 per row   the row's address is wave-uniform: read once per wave through the scalar cache, never per lane;
//   16-byte path         four 16-byte loads per lane, all issued before the four stores (4 VGPR quads in flight);
//   dword path           a source that is only 4-byte aligned (a view into a wider matrix at an odd column offset): sixteen
//                        dword loads per lane, then sixteen dword stores.  The branch is on the address: wave-uniform.
//
// A copy of bits: NaN payloads, -0.0 and subnormals survive.  No LDS, no scratch, no workspace, vector stores only.
#include "hmm_common.h"

namespace hmm {

typedef unsigned int gather_u32x4 __attribute__((ext_vector_type(4)));
// An address out of the table is a GLOBAL address: said so, the loads are global_load, not flat_load (no LDS / scratch aperture test).
typedef const __attribute__((address_space(1))) gather_u32x4* gather_src16;
typedef const __attribute__((address_space(1))) unsigned int* gather_src4;

constexpr int kGatherRowBytes = HMM_FEATURE_DIM * 4;
constexpr int64_t kGatherMaxBlocks = 1 << 20;                    // beyond 4 Mi rows a workgroup takes more than one group of four

__global__ __launch_bounds__(256) void rows_gather_kernel(const uint64_t* __restrict__ table, int64_t n, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < n; row += (int64_t)gridDim.x * 4) {
        const uint64_t a = table[row];                                        // wave-uniform index: one scalar load
        const uint64_t addr = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(a >> 32)) << 32) |
                              (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)a);
        float* dst = out + row * HMM_FEATURE_DIM;
        if ((addr & 15) == 0) {
            const gather_src16 src = (gather_src16)addr;
            gather_u32x4 v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = __builtin_nontemporal_load(src + j * 64 + lane);
#pragma unroll
            for (int j = 0; j < 4; ++j) reinterpret_cast<gather_u32x4*>(dst)[j * 64 + lane] = v[j];
        } else {
            const gather_src4 src = (gather_src4)addr;
            unsigned int v[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) v[j] = __builtin_nontemporal_load(src + j * 64 + lane);
#pragma unroll
            for (int j = 0; j < 16; ++j) reinterpret_cast<unsigned int*>(dst)[j * 64 + lane] = v[j];
        }
    }
}

}  // namespace hmm

using namespace hmm;

extern "C" int hmm_rows_gather(const uint64_t* src_row_ptrs_dev, int64_t n, int dim, float* out_dev, hmm_stream_t stream) {
    HMM_REQUIRE(dim == HMM_FEATURE_DIM, HMM_E_INVALID, "rows_gather: dim must be %d, got %d", HMM_FEATURE_DIM, dim);
    HMM_REQUIRE(n >= 0, HMM_E_INVALID, "rows_gather: negative count (n=%lld)", (long long)n);
    if (n == 0) return HMM_OK;                                                // nothing to write: no pointer is looked at
    HMM_REQUIRE(src_row_ptrs_dev && out_dev, HMM_E_INVALID, "rows_gather: null pointer (%s)",
                src_row_ptrs_dev ? "output" : "address table");
    HMM_REQUIRE(((uintptr_t)src_row_ptrs_dev & 7) == 0, HMM_E_INVALID, "rows_gather: the address table must be 8-byte aligned");
    HMM_REQUIRE(((uintptr_t)out_dev & 15) == 0, HMM_E_INVALID, "rows_gather: the output must be 16-byte aligned");
    static_assert(kGatherRowBytes == 4096, "one wave64 moves 64 lanes x 4 x 16 bytes");
    const int64_t blocks = (n + 3) / 4;
    rows_gather_kernel<<<(unsigned)(blocks > kGatherMaxBlocks ? kGatherMaxBlocks : blocks), 256, 0, static_cast<hipStream_t>(stream)>>>(
        src_row_ptrs_dev, n, out_dev);
    HMM_LAUNCH_CHECK();
    return HMM_OK;
}
