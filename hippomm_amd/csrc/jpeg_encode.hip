// Baseline JPEG encoding on gfx950: n frames of one geometry (packed u8 RGB, BGR or grey, resident) -> n complete files, each
// Pillow's Image.save(.., "JPEG", quality=q, subsampling=s) byte for byte.  The per-thread work is jpeg_encode_core.h (shared with
// the host model); this file is the thread mapping.  Five launches and one memset per call, cut where one stage needs all of the
// stage before it; no workgroup waits for another inside a launch.
//
//  (a) jpeg_fdct_kernel: colour transform, edge replication, chroma downsampling, level shift, forward DCT and quantisation.
//      8 threads per block: thread t fetches and transforms row t, then column t through LDS; the quantised block goes through
//      LDS once more into zigzag order and leaves as one 16-byte store per thread.  Blocks lie in scan order in the workspace.
//  (b) jpeg_size_kernel: one thread per block: its code length in bits.  The DC difference against the component's block before
//      it in the scan is read directly, there is no chain.  jpeg_scan_kernel: one workgroup per frame prefix-sums the lengths,
//      1024 per step with the total carried: the bit offset of every block and the frame's total.
//  (c) jpeg_emit_kernel: one thread per block writes the block's bits at its offset into the zeroed bitstream.  The first and
//      the last word a block touches are combined with an atomic OR (integer, order-independent: the bits do not depend on the
//      schedule); the last block also pads the last byte with ones.
//  (d) jpeg_stuff_kernel: one workgroup per frame.  16 bitstream bytes per thread and step: count the FF bytes, prefix-sum,
//      scatter behind the header with a 00 after every FF; then the header in front, FF D9 behind, length and status.  No byte at
//      or beyond the slot's end is written; a file that does not fit is reported as HMM_JPEG_ENCODE_OVERFLOW with its size.
// Integer arithmetic only, plain C++, vector stores only.
#include "hmm_common.h"
#include "jpeg_encode_core.h"

namespace hmm {

__constant__ JpegHuffEnc d_enc_huff[4] = {jpeg_huff_enc(kJpegStdDcLuma), jpeg_huff_enc(kJpegStdAcLuma), jpeg_huff_enc(kJpegStdDcChroma),
                                          jpeg_huff_enc(kJpegStdAcChroma)};

// Workspace of a call: [coefficients: n * blocks * 128 | bit offsets: n * (blocks + 1) u32, the last the total | bitstreams:
// n * bit_bytes], each part 256-byte aligned.
struct EncWorkspace {
    size_t coef_off, offs_off, bits_off, total;
};
inline EncWorkspace enc_workspace(const JpegEncLayout& L, int n) {
    EncWorkspace w;
    w.coef_off = 0;
    w.offs_off = align_up((size_t)n * L.blocks * kJpegBlockBytes, 256);
    w.bits_off = w.offs_off + align_up((size_t)n * ((size_t)L.blocks + 1) * 4, 256);
    w.total = w.bits_off + align_up((size_t)n * L.bit_bytes, 256);
    return w;
}

__global__ __launch_bounds__(kEncFdctBlocks * 8) void jpeg_fdct_kernel(const uint8_t* __restrict__ frames, int n, JpegEncLayout L,
                                                                       int channels, int bgr, const uint16_t* __restrict__ qtables,
                                                                       int16_t* __restrict__ coefs) {
    __shared__ int32_t s_ws[kEncFdctBlocks][64 + 1];
    __shared__ int16_t s_zz[kEncFdctBlocks][64];
    const int lb = threadIdx.x >> 3, t = threadIdx.x & 7;
    const int64_t g = (int64_t)blockIdx.x * kEncFdctBlocks + lb;
    const bool live = g < (int64_t)n * L.blocks;
    const int64_t f = live ? g / L.blocks : 0;
    const uint32_t b = live ? (uint32_t)(g - f * L.blocks) : 0;
    const EncBlock e = enc_block_at(L, b);
    if (live) {                                                        // pass 1: row t
        int32_t d[8], o[8];
        enc_sample_row(frames + f * ((int64_t)L.w * L.h * channels), L, channels, bgr, e.comp, e.bx, e.by, t, d);
        enc_fdct_1d(d, o, true);
#pragma unroll
        for (int k = 0; k < 8; ++k) s_ws[lb][t * 8 + k] = o[k];
    }
    __syncthreads();
    int32_t o[8];
    if (live) {                                                        // pass 2: column t
        int32_t d[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = s_ws[lb][k * 8 + t];
        enc_fdct_1d(d, o, false);
    }
    __syncthreads();
    if (live) {                                                        // quantise; s_ws now holds the block in natural order
        const uint16_t* q = qtables + (e.comp ? 64 : 0);
#pragma unroll
        for (int k = 0; k < 8; ++k) s_ws[lb][k * 8 + t] = (e.dummy && (k | t)) ? 0 : enc_quantise(o[k], q[k * 8 + t]);
    }
    __syncthreads();
    if (live) {
        int16_t* zz = &s_zz[lb][t * 8];
#pragma unroll
        for (int k = 0; k < 8; ++k) zz[k] = (int16_t)s_ws[lb][kJpegZigzag[t * 8 + k]];
        *reinterpret_cast<uint4*>(coefs + g * 64 + t * 8) = *reinterpret_cast<const uint4*>(zz);
    }
}

// Exclusive prefix sum of v over the workgroup's kEncScanTile threads; *total: the sum.  s: kEncScanTile / 64 + 1 words of LDS.
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* s, uint32_t* total) {
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t up = __shfl_up(inc, off, 64);
        if (lane >= (unsigned)off) inc += up;
    }
    __syncthreads();                                                   // s is free again (the previous step's readers are done)
    if (lane == 63) s[wave] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < kEncScanTile / 64; ++k) {
        const uint32_t x = s[k];
        before += k < (int)wave ? x : 0;
        all += x;
    }
    *total = all;
    return before + inc - v;
}

__device__ __forceinline__ void load_block(const int16_t* __restrict__ src, int16_t* zz) {
#pragma unroll
    for (int k = 0; k < 8; ++k) *reinterpret_cast<uint4*>(zz + 8 * k) = *reinterpret_cast<const uint4*>(src + 8 * k);
}

// The code length of every block in bits, into the slot of its bit offset.
__global__ __launch_bounds__(kEncEmitThreads) void jpeg_size_kernel(const int16_t* __restrict__ coefs, int n, JpegEncLayout L,
                                                                    uint32_t* __restrict__ offs) {
    const int64_t g = (int64_t)blockIdx.x * kEncEmitThreads + threadIdx.x;
    if (g >= (int64_t)n * L.blocks) return;
    const int64_t f = g / L.blocks;
    const uint32_t b = (uint32_t)(g - f * L.blocks);
    const int16_t* fc = coefs + f * (int64_t)L.blocks * 64;
    alignas(16) int16_t zz[64];
    load_block(fc + (int64_t)b * 64, zz);
    const int64_t pb = enc_pred_block(L, b);
    const int32_t pred = pb < 0 ? 0 : fc[pb * 64];
    const int table = (L.ncomp == 3 && b % (uint32_t)L.bpm >= (uint32_t)(L.hs * L.vs)) ? 2 : 0;
    EncBitCounter counter;
    enc_block_bits(zz, pred, d_enc_huff[table], d_enc_huff[table + 1], counter);
    offs[f * ((int64_t)L.blocks + 1) + b] = counter.bits;
}

// Lengths -> exclusive prefix sums in place, the frame's total behind them.
__global__ __launch_bounds__(kEncScanTile) void jpeg_scan_kernel(JpegEncLayout L, uint32_t* __restrict__ offs) {
    __shared__ uint32_t s_wave[kEncScanTile / 64 + 1];
    uint32_t* fo = offs + (int64_t)blockIdx.x * ((int64_t)L.blocks + 1);
    uint32_t carry = 0;
    for (uint32_t base = 0; base < L.blocks; base += kEncScanTile) {
        const uint32_t b = base + threadIdx.x;
        const uint32_t bits = b < L.blocks ? fo[b] : 0;
        uint32_t total;
        const uint32_t before = block_exclusive_scan(bits, s_wave, &total);
        if (b < L.blocks) fo[b] = carry + before;
        carry += total;
    }
    if (threadIdx.x == 0) fo[L.blocks] = carry;
}

struct DeviceWords {
    uint32_t* w;
    __device__ __forceinline__ void or_word(uint32_t i, uint32_t v) { atomicOr(w + i, v); }
    __device__ __forceinline__ void set_word(uint32_t i, uint32_t v) { w[i] = v; }
};

__global__ __launch_bounds__(kEncEmitThreads) void jpeg_emit_kernel(const int16_t* __restrict__ coefs, int n, JpegEncLayout L,
                                                                    const uint32_t* __restrict__ offs, uint8_t* __restrict__ bits) {
    const int64_t g = (int64_t)blockIdx.x * kEncEmitThreads + threadIdx.x;
    if (g >= (int64_t)n * L.blocks) return;
    const int64_t f = g / L.blocks;
    const uint32_t b = (uint32_t)(g - f * L.blocks);
    const int16_t* fc = coefs + f * (int64_t)L.blocks * 64;
    const uint32_t* fo = offs + f * ((int64_t)L.blocks + 1);
    const uint32_t total = fo[L.blocks];
    if (((uint64_t)total + 7) / 8 > L.bit_bytes) return;              // cannot happen (kJpegMaxBlockBits); the stuffing pass reports it
    alignas(16) int16_t zz[64];
    load_block(fc + (int64_t)b * 64, zz);
    const int64_t pb = enc_pred_block(L, b);
    const int32_t pred = pb < 0 ? 0 : fc[pb * 64];
    const int table = (L.ncomp == 3 && b % (uint32_t)L.bpm >= (uint32_t)(L.hs * L.vs)) ? 2 : 0;
    DeviceWords words{reinterpret_cast<uint32_t*>(bits + f * (int64_t)L.bit_bytes)};
    EncBitWriter<DeviceWords> writer(words, fo[b]);
    enc_block_bits(zz, pred, d_enc_huff[table], d_enc_huff[table + 1], writer);
    if (b + 1 == L.blocks) {
        const uint32_t pad = (8 - (total & 7)) & 7;
        if (pad) writer.put((1u << pad) - 1, pad);
    }
    writer.finish();
}

__global__ __launch_bounds__(kEncScanTile) void jpeg_stuff_kernel(const uint8_t* __restrict__ bits, JpegEncLayout L,
                                                                  const uint32_t* __restrict__ offs, const uint8_t* __restrict__ header,
                                                                  uint8_t* __restrict__ out, uint64_t out_stride, int32_t* __restrict__ status) {
    __shared__ uint32_t s_wave[kEncScanTile / 64 + 1];
    const int64_t f = blockIdx.x;
    const uint8_t* fb = bits + f * (int64_t)L.bit_bytes;
    uint8_t* fout = out + f * out_stride;
    const uint32_t total_bits = offs[f * ((int64_t)L.blocks + 1) + L.blocks];
    const bool fits = ((uint64_t)total_bits + 7) / 8 <= L.bit_bytes;
    const uint32_t used = fits ? (total_bits + 7) / 8 : 0;
    for (uint32_t i = threadIdx.x; i < L.header_bytes && i < out_stride; i += kEncScanTile) fout[i] = header[i];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < used; base += kEncScanTile * kEncStuffBytes) {
        const uint32_t first = base + threadIdx.x * kEncStuffBytes;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (first < used) v = *reinterpret_cast<const uint4*>(fb + first);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        const uint32_t mine = enc_count_ff(w, first, used);
        uint32_t total;
        const uint32_t before = block_exclusive_scan(mine, s_wave, &total);
        enc_scatter(w, first, used, carry + before, L.header_bytes, fout, out_stride);
        carry += total;
    }
    if (threadIdx.x == 0) {
        const uint64_t size = (uint64_t)L.header_bytes + used + carry + 2;
        const bool ok = fits && size <= out_stride;
        if (ok) {
            fout[size - 2] = 0xFF;
            fout[size - 1] = 0xD9;
        }
        status[2 * f] = ok ? HMM_JPEG_ENCODED : HMM_JPEG_ENCODE_OVERFLOW;
        status[2 * f + 1] = (int32_t)(size > 0x7FFFFFFF ? 0x7FFFFFFF : size);
    }
}

}  // namespace hmm

using namespace hmm;

namespace {
bool enc_layout_of(const int32_t* geometry, JpegEncLayout* L) {
    return geometry && jpeg_enc_layout(geometry[0], geometry[1], geometry[2], geometry[3], geometry[4], L);
}
}  // namespace

extern "C" size_t hmm_jpeg_encode_workspace_bytes(const int32_t* geometry, int n) {
    JpegEncLayout L;
    if (n < 1 || !enc_layout_of(geometry, &L)) return 0;
    return enc_workspace(L, n).total;
}

// Every file of the geometry is at most this long: the header, FF D9, and twice the bitstream's capacity -- each block is at most
// kJpegMaxBlockBits (jpeg_layout.h: 22 DC bits and 26 for each of the 63 AC positions), the last byte is padded, and stuffing adds
// at most one 00 per byte.
extern "C" size_t hmm_jpeg_encode_bound(const int32_t* geometry) {
    JpegEncLayout L;
    if (!enc_layout_of(geometry, &L)) return 0;
    return (size_t)L.header_bytes + 2 * (((size_t)L.blocks * kJpegMaxBlockBits + 7) / 8) + 2;
}

extern "C" int hmm_jpeg_encode(const uint8_t* frames_dev, int n, const int32_t* geometry, int channels, int channel_order,
                               const uint16_t* qtables_dev, const uint8_t* header_dev, size_t header_bytes, uint8_t* out_dev,
                               size_t out_stride, int32_t* status_dev, void* workspace_dev, size_t workspace_bytes,
                               hmm_stream_t stream) {
    HMM_REQUIRE(frames_dev && geometry && qtables_dev && header_dev && out_dev && status_dev && workspace_dev, HMM_E_INVALID,
                "jpeg_encode: null pointer");
    HMM_REQUIRE(n >= 0, HMM_E_INVALID, "jpeg_encode: negative frame count %d", n);
    JpegEncLayout L;
    HMM_REQUIRE(enc_layout_of(geometry, &L), HMM_E_INVALID,
                "jpeg_encode: bad geometry (%d x %d, %d components, sampling %d x %d): sides of 1..65535, 1 or 3 components, "
                "4:4:4, 4:2:2 or 4:2:0, and a frame small enough for 32-bit bit offsets",
                geometry[0], geometry[1], geometry[2], geometry[3], geometry[4]);
    HMM_REQUIRE(channels == L.ncomp, HMM_E_INVALID, "jpeg_encode: %d channels for %d components", channels, L.ncomp);
    HMM_REQUIRE(channel_order == HMM_JPEG_ORDER_RGB || channel_order == HMM_JPEG_ORDER_BGR, HMM_E_INVALID,
                "jpeg_encode: channel order %d (0 RGB, 1 BGR)", channel_order);
    HMM_REQUIRE(header_bytes == L.header_bytes, HMM_E_INVALID, "jpeg_encode: header of %zu bytes, %u expected for this geometry",
                header_bytes, L.header_bytes);
    HMM_REQUIRE(((uintptr_t)qtables_dev & 1) == 0 && ((uintptr_t)status_dev & 3) == 0 && ((uintptr_t)workspace_dev & 15) == 0,
                HMM_E_INVALID, "jpeg_encode: the workspace must be 16-byte aligned, the status 4-byte and the tables 2-byte aligned");
    HMM_REQUIRE(out_stride >= 1, HMM_E_INVALID, "jpeg_encode: output stride of 0 bytes");
    if (n == 0) return HMM_OK;
    const EncWorkspace ws = enc_workspace(L, n);
    HMM_REQUIRE(workspace_bytes >= ws.total, HMM_E_WORKSPACE, "jpeg_encode: workspace of %zu bytes, %zu needed", workspace_bytes, ws.total);
    const int64_t blocks = (int64_t)n * L.blocks;
    const int64_t fdct_groups = (blocks + kEncFdctBlocks - 1) / kEncFdctBlocks;
    HMM_REQUIRE(fdct_groups <= 0x7FFFFFFF, HMM_E_INVALID, "jpeg_encode: %lld blocks in one call is too many", (long long)blocks);
    hipStream_t st = static_cast<hipStream_t>(stream);
    uint8_t* base = static_cast<uint8_t*>(workspace_dev);
    int16_t* coefs = reinterpret_cast<int16_t*>(base + ws.coef_off);
    uint32_t* offs = reinterpret_cast<uint32_t*>(base + ws.offs_off);
    uint8_t* bits = base + ws.bits_off;
    HMM_HIP_CHECK(hipMemsetAsync(bits, 0, (size_t)n * L.bit_bytes, st));
    jpeg_fdct_kernel<<<(unsigned)fdct_groups, kEncFdctBlocks * 8, 0, st>>>(frames_dev, n, L, channels, channel_order == HMM_JPEG_ORDER_BGR,
                                                                           qtables_dev, coefs);
    HMM_LAUNCH_CHECK();
    const unsigned block_groups = (unsigned)((blocks + kEncEmitThreads - 1) / kEncEmitThreads);
    jpeg_size_kernel<<<block_groups, kEncEmitThreads, 0, st>>>(coefs, n, L, offs);
    HMM_LAUNCH_CHECK();
    jpeg_scan_kernel<<<(unsigned)n, kEncScanTile, 0, st>>>(L, offs);
    HMM_LAUNCH_CHECK();
    jpeg_emit_kernel<<<block_groups, kEncEmitThreads, 0, st>>>(coefs, n, L, offs, bits);
    HMM_LAUNCH_CHECK();
    jpeg_stuff_kernel<<<(unsigned)n, kEncScanTile, 0, st>>>(bits, L, offs, header_dev, out_dev, (uint64_t)out_stride, status_dev);
    HMM_LAUNCH_CHECK();
    return HMM_OK;
}
