// Device entropy pass of the baseline JPEG decoder: bitstream slots (jpeg_host.cpp: hmm_jpeg_prepare_entropy) -> the coefficient
// slots hmm_jpeg_decode_coefs writes, byte for byte, on gfx950.  The algorithm and every function that decodes are in
// jpeg_entropy_core.h, shared with the CPU model; this file holds the two kernels and the launch.
//
//  (a) jpeg_entropy_kernel: one workgroup of kEntropyThreads per frame.  Huffman tables in LDS; the fixed-point rounds with a
//      barrier between a round and the hand-over of exit states (every thread reaches every barrier: the loop condition is a
//      workgroup-wide OR); block-count prefix sum; the write pass into full-frame coefficients in the workspace; DC prefix sum
//      and walk; the frame's status, the slot's quantisation header and its zero padding.
//  (b) jpeg_entropy_finish_kernel: one thread per block of every frame: the host's per-block refusals, and the copy of the
//      blocks the window keeps into the slot.
// Integer arithmetic only, no scratch, vector stores only.
#include "hmm_common.h"
#include "jpeg_entropy_core.h"

namespace hmm {

constexpr int kEntropyChunk = 32;                 // frames per launch: bounds the workspace
constexpr int kFinishThreads = 256;

struct EntropyArgs {
    const uint8_t* bitslots;
    size_t bitslot_stride;
    uint8_t* slots;
    size_t slot_stride;
    int32_t* status;                              // [n][2]
    uint8_t* workspace;
    EntropyWorkspace ws;
    JpegLayout L;
    int hmax, vmax, mcux;
    uint32_t total_blocks;
};

__device__ __forceinline__ uint32_t exclusive_prefix(const uint32_t* s, uint32_t t) {
    uint32_t sum = 0;
    for (uint32_t k = 0; k < t; ++k) sum += s[k];
    return sum;
}

__global__ __launch_bounds__(kEntropyThreads) void jpeg_entropy_kernel(EntropyArgs a) {
    __shared__ EntropyHuff s_huff[4];
    __shared__ uint64_t s_boundary[kEntropyThreads];
    __shared__ uint32_t s_sum[4][kEntropyThreads];
    __shared__ uint32_t s_bad, s_end;
    const uint32_t t = threadIdx.x;
    const int f = blockIdx.x;
    const uint8_t* bs = a.bitslots + (size_t)f * a.bitslot_stride;
    const int32_t* head = reinterpret_cast<const int32_t*>(bs);
    uint8_t* slot = a.slots + (size_t)f * a.slot_stride;
    uint8_t* wsf = a.workspace + (size_t)f * a.ws.frame_bytes;

    // The slot's header and padding do not depend on the data.
    if (t < kJpegQtBytes / 16) reinterpret_cast<uint4*>(slot)[t] = reinterpret_cast<const uint4*>(bs + kEntropyQtOff)[t];
    for (int64_t o = kJpegQtBytes + a.L.block_off[a.L.ncomp] * kJpegBlockBytes + (int64_t)t * 16; o < a.L.slot_bytes; o += kEntropyThreads * 16)
        *reinterpret_cast<uint4*>(slot + o) = make_uint4(0, 0, 0, 0);

    const uint32_t nbytes = (uint32_t)head[kEhBytes];
    const bool header_ok = (uint32_t)head[kEhMagic] == kEntropyMagic && head[kEhComps] == a.L.ncomp && head[kEhHmax] == a.hmax &&
                           head[kEhVmax] == a.vmax && nbytes <= kEntropyMaxBytes &&
                           (size_t)kEntropyDataOff + ((size_t)nbytes + 3) / 4 * 4 <= a.bitslot_stride &&
                           entropy_subsequences(nbytes * 8) <= a.ws.max_sub;
    if (!header_ok) {                             // uniform: every thread read the same words
        if (t == 0) {
            a.status[2 * f] = HMM_JPEG_UNSUPPORTED;
            a.status[2 * f + 1] = 0;
        }
        return;
    }
    for (uint32_t k = t; k < 4 * sizeof(EntropyHuff) / 16; k += kEntropyThreads)
        reinterpret_cast<uint4*>(s_huff)[k] = reinterpret_cast<const uint4*>(bs + kEntropyHuffOff)[k];
    if (t == 0) {
        s_bad = 0;
        s_end = kNoEnd;
    }

    EntropyCtx c;
    c.words = reinterpret_cast<const uint32_t*>(bs + kEntropyDataOff);
    c.nwords = (nbytes + 3) / 4;
    c.total_bits = nbytes * 8;
    c.huff = s_huff;
    c.selectors = (uint32_t)head[kEhSelectors];
    c.ncomp = a.L.ncomp;
    c.hv = a.L.ncomp == 3 ? a.hmax * a.vmax : 1;
    c.bpm = a.L.ncomp == 3 ? c.hv + 2 : 1;
    c.total_blocks = a.total_blocks;
    c.nsub = entropy_subsequences(c.total_bits);
    c.per = (c.nsub + kEntropyThreads - 1) / kEntropyThreads;
    c.entry = reinterpret_cast<uint64_t*>(wsf + a.ws.entry_off);
    c.count = reinterpret_cast<uint32_t*>(wsf + a.ws.count_off);
    c.dirty = reinterpret_cast<uint32_t*>(wsf + a.ws.dirty_off);
    c.coef = reinterpret_cast<int16_t*>(wsf);

    entropy_init(c, t, s_boundary);
    __syncthreads();
    uint32_t rounds = 0;
    bool converged = false;
    while (rounds <= c.nsub) {                    // the proven bound: subsequences + 1 rounds
        ++rounds;
        entropy_round(c, t, s_boundary);
        __syncthreads();
        const int changed = entropy_sync(c, t, s_boundary);
        if (!__syncthreads_or(changed)) {
            converged = true;
            break;
        }
    }

    s_sum[0][t] = entropy_thread_blocks(c, t);
    __syncthreads();
    ThreadOut th;
    entropy_write(c, t, exclusive_prefix(s_sum[0], t), th);
    s_sum[1][t] = th.d0;
    s_sum[2][t] = th.d1;
    s_sum[3][t] = th.d2;
    if (th.end_bit != kNoEnd) s_end = th.end_bit;            // one thread at the most ends the frame
    __syncthreads();
    uint32_t bad = th.bad | entropy_dc_walk(c, th, (int32_t)exclusive_prefix(s_sum[1], t), (int32_t)exclusive_prefix(s_sum[2], t),
                                            (int32_t)exclusive_prefix(s_sum[3], t));
    if (bad) s_bad = 1;
    __syncthreads();
    if (t == 0) {
        a.status[2 * f] = (converged && !s_bad && entropy_end_ok(s_end, c.total_bits)) ? HMM_JPEG_DECODED : HMM_JPEG_UNSUPPORTED;
        a.status[2 * f + 1] = (int32_t)rounds;
    }
}

__global__ __launch_bounds__(kFinishThreads) void jpeg_entropy_finish_kernel(EntropyArgs a, int n) {
    const int64_t g = (int64_t)blockIdx.x * kFinishThreads + threadIdx.x;
    if (g >= (int64_t)n * a.total_blocks) return;
    const int f = (int)(g / a.total_blocks);
    const uint32_t b = (uint32_t)(g - (int64_t)f * a.total_blocks);
    if (a.status[2 * f] != HMM_JPEG_DECODED) return;         // refused by the entropy kernel: the slot is not used
    const int hv = a.L.ncomp == 3 ? a.hmax * a.vmax : 1, bpm = a.L.ncomp == 3 ? hv + 2 : 1;
    const bool bad = finish_block(reinterpret_cast<const int16_t*>(a.workspace + (size_t)f * a.ws.frame_bytes),
                                  reinterpret_cast<const uint16_t*>(a.bitslots + (size_t)f * a.bitslot_stride + kEntropyQtOff), a.L,
                                  a.mcux, hv, bpm, b, a.slots + (size_t)f * a.slot_stride);
    // Raising the status with a maximum, and the plain read above (a stale DECODED only costs a copy into a slot that is refused
    // anyway), rely on the order of the two constants.
    static_assert(HMM_JPEG_UNSUPPORTED > HMM_JPEG_DECODED, "the finish kernel raises a frame's status with atomicMax");
    if (bad) atomicMax(&a.status[2 * f], (int32_t)HMM_JPEG_UNSUPPORTED);
}

}  // namespace hmm

using namespace hmm;

namespace {
bool geometry_ok(const int32_t* g) {
    return g && g[0] >= 1 && g[1] >= 1 && g[0] <= 65535 && g[1] <= 65535 && (g[2] == 1 || g[2] == 3) &&
           (g[2] == 1 || ((g[3] == 1 || g[3] == 2) && (g[4] == 1 || g[4] == 2) && !(g[3] == 1 && g[4] == 2)));
}
}  // namespace

extern "C" size_t hmm_jpeg_entropy_workspace_bytes(const int32_t* geometry, int n, size_t max_entropy_bytes) {
    if (n < 1 || !geometry_ok(geometry)) return 0;
    const EntropyWorkspace w = entropy_workspace(entropy_total_blocks(geometry[0], geometry[1], geometry[2], geometry[3], geometry[4]),
                                                 max_entropy_bytes);
    return (size_t)(n < kEntropyChunk ? n : kEntropyChunk) * w.frame_bytes;
}

extern "C" int hmm_jpeg_decode_coefs_device(const void* bitslots_dev, int n, size_t bitslot_stride, const int32_t* geometry, int x0,
                                            int y0, int w, int h, void* coef_slots_dev, size_t coef_slot_stride, int32_t* status_dev,
                                            void* workspace_dev, size_t workspace_bytes, hmm_stream_t stream) {
    HMM_REQUIRE(n >= 0, HMM_E_INVALID, "jpeg_decode_coefs_device: negative frame count %d", n);
    HMM_REQUIRE(bitslots_dev && geometry && coef_slots_dev && status_dev && workspace_dev, HMM_E_INVALID,
                "jpeg_decode_coefs_device: null pointer");
    HMM_REQUIRE(geometry_ok(geometry), HMM_E_INVALID, "jpeg_decode_coefs_device: bad geometry");
    EntropyArgs a;
    HMM_REQUIRE(jpeg_layout(geometry[0], geometry[1], geometry[2], geometry[3], geometry[4], x0, y0, w, h, &a.L), HMM_E_INVALID,
                "jpeg_decode_coefs_device: window (%d, %d, %d, %d) outside the %d x %d frame", x0, y0, w, h, geometry[0], geometry[1]);
    HMM_REQUIRE(((uintptr_t)bitslots_dev & 15) == 0 && ((uintptr_t)coef_slots_dev & 15) == 0 && ((uintptr_t)workspace_dev & 15) == 0 &&
                    ((uintptr_t)status_dev & 3) == 0,
                HMM_E_INVALID, "jpeg_decode_coefs_device: slots and workspace must be 16-byte aligned, the status words 4-byte aligned");
    HMM_REQUIRE(bitslot_stride >= (size_t)kEntropyDataOff + kEntropyPad && bitslot_stride % 16 == 0, HMM_E_INVALID,
                "jpeg_decode_coefs_device: bitstream slot stride %zu (>= %d and a multiple of 16 needed)", bitslot_stride,
                kEntropyDataOff + kEntropyPad);
    HMM_REQUIRE(coef_slot_stride >= (size_t)a.L.slot_bytes && coef_slot_stride % 16 == 0, HMM_E_INVALID,
                "jpeg_decode_coefs_device: coefficient slot stride %zu (>= %lld and a multiple of 16 needed)", coef_slot_stride,
                (long long)a.L.slot_bytes);
    if (n == 0) return HMM_OK;
    const size_t need = hmm_jpeg_entropy_workspace_bytes(geometry, n, bitslot_stride);
    HMM_REQUIRE(workspace_bytes >= need, HMM_E_WORKSPACE, "jpeg_decode_coefs_device: workspace of %zu bytes, %zu needed",
                workspace_bytes, need);
    a.hmax = geometry[2] == 3 ? geometry[3] : 1;
    a.vmax = geometry[2] == 3 ? geometry[4] : 1;
    a.mcux = jpeg_cdiv(geometry[0], 8 * a.hmax);
    a.total_blocks = entropy_total_blocks(geometry[0], geometry[1], geometry[2], geometry[3], geometry[4]);
    a.ws = entropy_workspace(a.total_blocks, bitslot_stride);
    a.bitslot_stride = bitslot_stride;
    a.slot_stride = coef_slot_stride;
    a.workspace = static_cast<uint8_t*>(workspace_dev);
    hipStream_t st = static_cast<hipStream_t>(stream);
    for (int f0 = 0; f0 < n; f0 += kEntropyChunk) {
        const int m = n - f0 < kEntropyChunk ? n - f0 : kEntropyChunk;
        a.bitslots = static_cast<const uint8_t*>(bitslots_dev) + (size_t)f0 * bitslot_stride;
        a.slots = static_cast<uint8_t*>(coef_slots_dev) + (size_t)f0 * coef_slot_stride;
        a.status = status_dev + 2 * (size_t)f0;
        // a block that straddles two subsequences is written by two threads: zero the coefficients first
        HMM_HIP_CHECK(hipMemsetAsync(a.workspace, 0, (size_t)m * a.ws.frame_bytes, st));
        jpeg_entropy_kernel<<<(unsigned)m, kEntropyThreads, 0, st>>>(a);
        HMM_LAUNCH_CHECK();
        const int64_t groups = ((int64_t)m * a.total_blocks + kFinishThreads - 1) / kFinishThreads;
        HMM_REQUIRE(groups <= 0x7FFFFFFF, HMM_E_INVALID, "jpeg_decode_coefs_device: frame too large");
        jpeg_entropy_finish_kernel<<<(unsigned)groups, kFinishThreads, 0, st>>>(a, m);
        HMM_LAUNCH_CHECK();
    }
    return HMM_OK;
}
