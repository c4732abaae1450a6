// Device half of the baseline JPEG decoder: coefficient slots (jpeg_host.cpp's entropy pass) -> packed RGB u8 on gfx950, with
// the arithmetic libjpeg-turbo runs under Pillow's defaults, so the pixels are Image.open(path).convert("RGB")'s to the bit.
//
//  (a) jpeg_idct_kernel: dequantise and JDCT_ISLOW (jidctint.c: CONST_BITS 13, PASS1_BITS 2, DESCALE rounding, the post-IDCT
//      range limit -- see idct_limit) into u8 sample planes in the workspace.  8 threads per block: thread t loads
//      coefficient row t, runs column t of pass 1 and row t of pass 2 through LDS, and writes its 8 samples with one 8-byte store.
//      The products are 64-bit like the C code's JLONG; the host refuses blocks whose first-pass values would leave int16, where
//      libjpeg-turbo's SIMD and C paths would part (jpeg_host.cpp, kColumnBound).
//  (b) jpeg_color_kernel: chroma upsampling -- jdsample.c's triangle filter (h2v1: (3 a + b + 1 | 2) >> 2; h2v2: the same on
//      column sums 3 a + b of the nearer and the farther row, (3 s + t + 8 | 7) >> 4) over the component's downsampled width and
//      height, edge samples and the first / last row replicated; plain replication when the downsampled width is 2 or less, as
//      libjpeg-turbo chooses -- then jdcolor.c's fixed-point YCbCr -> RGB (SCALEBITS 16) and packing.  4 pixels per thread, three
//      dword stores.
//  (c) jpeg_encoded_idct_kernel: (a) for frames this process has just encoded -- it reads the quantised blocks hmm_jpeg_encode
//      left in its workspace (scan order, zigzag order) and the encoder's two tables instead of coefficient slots, so the pixels a
//      decoder would recover from the file are made without the file: hmm_jpeg_encoded_pixels.  (b) follows unchanged.
// Integer arithmetic only, no scratch, vector stores only; HBM traffic is a few MB per 1080p frame.
#include "hmm_common.h"
#include "jpeg_layout.h"

namespace hmm {

constexpr int kIdctBlocks = 32;                   // blocks per workgroup, 8 threads each
constexpr int kColorThreads = 256;

__device__ __forceinline__ int64_t descale(int64_t x, int n) { return (x + ((int64_t)1 << (n - 1))) >> n; }

// jidctint.c's butterfly: the eight outputs before descaling, in output order.
__device__ __forceinline__ void islow_1d(int64_t d0, int64_t d1, int64_t d2, int64_t d3, int64_t d4, int64_t d5, int64_t d6,
                                         int64_t d7, int64_t* o) {
    int64_t z1 = (d2 + d6) * 4433;                                  // FIX_0_541196100
    const int64_t tmp2 = z1 + d6 * -15137;                          // FIX_1_847759065
    const int64_t tmp3 = z1 + d2 * 6270;                            // FIX_0_765366865
    const int64_t tmp0 = (d0 + d4) * 8192, tmp1 = (d0 - d4) * 8192;
    const int64_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    int64_t t0 = d7, t1 = d5, t2 = d3, t3 = d1;
    z1 = t0 + t3;
    int64_t z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
    const int64_t z5 = (z3 + z4) * 9633;                            // FIX_1_175875602
    t0 *= 2446;                                                     // FIX_0_298631336
    t1 *= 16819;                                                    // FIX_2_053119869
    t2 *= 25172;                                                    // FIX_3_072711026
    t3 *= 12299;                                                    // FIX_1_501321110
    z1 *= -7373;                                                    // FIX_0_899976223
    z2 *= -20995;                                                   // FIX_2_562915447
    z3 = z3 * -16069 + z5;                                          // FIX_1_961570560
    z4 = z4 * -3196 + z5;                                           // FIX_0_390180644
    t0 += z1 + z3;
    t1 += z2 + z4;
    t2 += z2 + z3;
    t3 += z1 + z4;
    o[0] = tmp10 + t3;
    o[7] = tmp10 - t3;
    o[1] = tmp11 + t2;
    o[6] = tmp11 - t2;
    o[2] = tmp12 + t1;
    o[5] = tmp12 - t1;
    o[3] = tmp13 + t0;
    o[4] = tmp13 - t0;
}

// The post-IDCT range limit as libjpeg-turbo's SIMD IDCT (what Pillow runs) applies it: x + 128 saturated to [0, 255].  It equals
// jidctint.c's table lookup (index x & 1023) for every |x| < 384, i.e. every value a file from an 8-bit encoder produces; beyond,
// the table wraps and the SIMD code saturates, and Pillow's pixels are the SIMD code's.
__device__ __forceinline__ uint32_t idct_limit(int64_t x) { return (uint32_t)(x < -128 ? 0 : x > 127 ? 255 : x + 128); }

// What both IDCT kernels run once coefficient row t of every block lies in coef (natural order, LDS): column t of pass 1
// dequantised by q, row t of pass 2, the range limit, and the row's 8 samples as one 8-byte store to dst.  Every thread of the
// workgroup calls it (the barriers are inside); threads that are not live only take part in the barriers.
__device__ __forceinline__ void idct_block(bool live, const int16_t* coef, int32_t* ws, int t, const uint16_t* __restrict__ q,
                                           uint8_t* __restrict__ dst) {
    __syncthreads();
    if (live) {                                                     // pass 1: column t, dequantised
        int64_t d[8], o[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = (int64_t)coef[k * 8 + t] * (int64_t)q[k * 8 + t];
        islow_1d(d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], o);
#pragma unroll
        for (int k = 0; k < 8; ++k) ws[k * 8 + t] = (int32_t)descale(o[k], 13 - 2);
    }
    __syncthreads();
    if (live) {                                                     // pass 2: row t
        const int32_t* w = &ws[t * 8];
        int64_t o[8];
        islow_1d(w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], o);
        uint2 px;
        px.x = idct_limit(descale(o[0], 18)) | idct_limit(descale(o[1], 18)) << 8 | idct_limit(descale(o[2], 18)) << 16 |
               idct_limit(descale(o[3], 18)) << 24;
        px.y = idct_limit(descale(o[4], 18)) | idct_limit(descale(o[5], 18)) << 8 | idct_limit(descale(o[6], 18)) << 16 |
               idct_limit(descale(o[7], 18)) << 24;
        *reinterpret_cast<uint2*>(dst) = px;
    }
}

// Block b of a frame's stored rectangles: its component, its place (bx, by) in that rectangle, and row t of it in the planes.
struct IdctBlock {
    int c, bx, by;
};
__device__ __forceinline__ IdctBlock idct_block_at(const JpegLayout& L, int64_t b) {
    IdctBlock e;
    e.c = b < L.block_off[1] ? 0 : (b < L.block_off[2] ? 1 : 2);
    const int64_t local = b - L.block_off[e.c];
    e.bx = (int)(local % L.nbx[e.c]);
    e.by = (int)(local / L.nbx[e.c]);
    return e;
}
__device__ __forceinline__ uint8_t* idct_row(uint8_t* __restrict__ planes, const JpegLayout& L, int64_t f, const IdctBlock& e, int t) {
    return planes + f * L.plane_off[L.ncomp] + L.plane_off[e.c] + (int64_t)(e.by * 8 + t) * (L.nbx[e.c] * 8) + e.bx * 8;
}

__global__ __launch_bounds__(kIdctBlocks * 8) void jpeg_idct_kernel(const uint8_t* __restrict__ slots, int64_t slot_stride, int n,
                                                                    JpegLayout L, uint8_t* __restrict__ planes) {
    __shared__ int16_t s_coef[kIdctBlocks][64];
    __shared__ int32_t s_ws[kIdctBlocks][64 + 1];
    const int lb = threadIdx.x >> 3, t = threadIdx.x & 7;
    const int64_t per = L.block_off[L.ncomp];
    const int64_t g = (int64_t)blockIdx.x * kIdctBlocks + lb;
    const bool live = g < (int64_t)n * per;
    const int64_t f = live ? g / per : 0, b = live ? g - f * per : 0;
    const IdctBlock e = idct_block_at(L, b);
    const uint8_t* slot = slots + f * slot_stride;
    if (live) {
        const uint4 row = *reinterpret_cast<const uint4*>(slot + kJpegQtBytes + b * kJpegBlockBytes + t * 16);
        *reinterpret_cast<uint4*>(&s_coef[lb][t * 8]) = row;
    }
    idct_block(live, s_coef[lb], s_ws[lb], t, reinterpret_cast<const uint16_t*>(slot) + 64 * e.c, idct_row(planes, L, f, e, t));
}

// The same planes from the workspace a finished hmm_jpeg_encode call left behind: the quantised blocks of every frame, int16[64]
// in zigzag order, in scan order (E), DC values absolute.  Block (gx, gy) of a component's grid is looked up in the scan -- a
// colour MCU is hs x vs luma blocks row by row, then Cb, then Cr; a grey MCU is one block -- and the zigzag is undone while the
// 16-byte row (zigzag positions 8 t .. 8 t + 7) is staged into LDS.  qtables: uint16[2][64], natural order (luma, chroma).
__global__ __launch_bounds__(kIdctBlocks * 8) void jpeg_encoded_idct_kernel(const int16_t* __restrict__ coefs, int n, JpegLayout L,
                                                                            JpegEncLayout E, const uint16_t* __restrict__ qtables,
                                                                            uint8_t* __restrict__ planes) {
    __shared__ int16_t s_coef[kIdctBlocks][64];
    __shared__ int32_t s_ws[kIdctBlocks][64 + 1];
    const int lb = threadIdx.x >> 3, t = threadIdx.x & 7;
    const int64_t per = L.block_off[L.ncomp];
    const int64_t g = (int64_t)blockIdx.x * kIdctBlocks + lb;
    const bool live = g < (int64_t)n * per;
    const int64_t f = live ? g / per : 0, b = live ? g - f * per : 0;
    const IdctBlock e = idct_block_at(L, b);
    if (live) {
        const int gx = L.bx0[e.c] + e.bx, gy = L.by0[e.c] + e.by;
        int64_t src;
        if (E.ncomp == 1)
            src = (int64_t)gy * E.mcux + gx;
        else if (e.c == 0)
            src = ((int64_t)(gy / E.vs) * E.mcux + gx / E.hs) * E.bpm + (gy % E.vs) * E.hs + gx % E.hs;
        else
            src = ((int64_t)gy * E.mcux + gx) * E.bpm + E.hs * E.vs + (e.c - 1);
        const uint4 row = *reinterpret_cast<const uint4*>(coefs + (f * (int64_t)E.blocks + src) * 64 + t * 8);
        const uint32_t w[4] = {row.x, row.y, row.z, row.w};
#pragma unroll
        for (int k = 0; k < 8; ++k) s_coef[lb][kJpegZigzag[t * 8 + k]] = (int16_t)(w[k >> 1] >> ((k & 1) * 16));
    }
    idct_block(live, s_coef[lb], s_ws[lb], t, qtables + (e.c ? 64 : 0), idct_row(planes, L, f, e, t));
}

// Sample (sx, sy) of component c (component coordinates; inside the stored rectangle by construction of the layout).
__device__ __forceinline__ int sample(const uint8_t* __restrict__ fp, const JpegLayout& L, int c, int sx, int sy) {
    return fp[L.plane_off[c] + (int64_t)(sy - L.by0[c] * 8) * (L.nbx[c] * 8) + (sx - L.bx0[c] * 8)];
}

__device__ __forceinline__ int chroma(const uint8_t* __restrict__ fp, const JpegLayout& L, int c, int X, int Y) {
    if (L.rx == 1) return sample(fp, L, c, X, Y);
    const int i = X >> 1, odd = X & 1;
    const int j = L.ry == 2 ? Y >> 1 : Y;
    if (!L.fancy) return sample(fp, L, c, i, j);
    const int in = odd ? min(i + 1, L.cw[c] - 1) : max(i - 1, 0);
    if (L.ry == 1) return (3 * sample(fp, L, c, i, j) + sample(fp, L, c, in, j) + 1 + odd) >> 2;
    const int jn = (Y & 1) ? min(j + 1, L.ch[c] - 1) : max(j - 1, 0);
    const int near = 3 * sample(fp, L, c, i, j) + sample(fp, L, c, i, jn);
    const int far = 3 * sample(fp, L, c, in, j) + sample(fp, L, c, in, jn);
    return (3 * near + far + 8 - odd) >> 4;
}

__device__ __forceinline__ uint32_t clamp_u8(int v) { return (uint32_t)min(max(v, 0), 255); }

// Window pixel (X, Y) of the frame whose planes start at fp -> packed R | G << 8 | B << 16.
__device__ __forceinline__ uint32_t rgb_at(const uint8_t* __restrict__ fp, const JpegLayout& L, int X, int Y) {
    const int y = sample(fp, L, 0, X, Y);
    if (L.ncomp == 1) return (uint32_t)y * 0x010101u;
    const int cb = chroma(fp, L, 1, X, Y) - 128, cr = chroma(fp, L, 2, X, Y) - 128;
    const uint32_t R = clamp_u8(y + ((91881 * cr + 32768) >> 16));                   // FIX(1.40200)
    const uint32_t G = clamp_u8(y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));     // FIX(0.34414), FIX(0.71414)
    const uint32_t B = clamp_u8(y + ((116130 * cb + 32768) >> 16));                  // FIX(1.77200)
    return R | G << 8 | B << 16;
}

// Walks the flat (n, h, w) window pixel by pixel from one division: frame, row and column advance with carries.
struct PixelCursor {
    int64_t f;
    int x, y;
    __device__ __forceinline__ PixelCursor(const JpegLayout& L, int64_t p) {
        const int64_t hw = (int64_t)L.w * L.h;
        f = p / hw;
        const uint32_t r = (uint32_t)(p - f * hw);                  // hw < 2^32: w, h <= 65535
        y = (int)(r / (uint32_t)L.w);
        x = (int)(r - (uint32_t)y * (uint32_t)L.w);
    }
    __device__ __forceinline__ uint32_t rgb(const uint8_t* __restrict__ planes, const JpegLayout& L) const {
        return rgb_at(planes + f * L.plane_off[L.ncomp], L, L.x0 + x, L.y0 + y);
    }
    __device__ __forceinline__ void next(const JpegLayout& L) {
        if (++x == L.w) {
            x = 0;
            if (++y == L.h) {
                y = 0;
                ++f;
            }
        }
    }
};

__global__ __launch_bounds__(kColorThreads) void jpeg_color_kernel(const uint8_t* __restrict__ planes, JpegLayout L, int n,
                                                                   uint8_t* __restrict__ out) {
    const int64_t total = (int64_t)n * L.w * L.h;
    const int64_t p0 = ((int64_t)blockIdx.x * kColorThreads + threadIdx.x) * 4;
    if (p0 >= total) return;
    PixelCursor cur(L, p0);
    if (p0 + 4 <= total) {
        const uint32_t a = cur.rgb(planes, L);
        cur.next(L);
        const uint32_t b = cur.rgb(planes, L);
        cur.next(L);
        const uint32_t c = cur.rgb(planes, L);
        cur.next(L);
        const uint32_t d = cur.rgb(planes, L);
        uint32_t* dst = reinterpret_cast<uint32_t*>(out + p0 * 3);                 // 12 p0 bytes in: dword aligned
        dst[0] = a | b << 24;
        dst[1] = b >> 8 | c << 16;
        dst[2] = c >> 16 | d << 8;
    } else {
        for (int64_t p = p0; p < total; ++p, cur.next(L)) {
            const uint32_t v = cur.rgb(planes, L);
            out[3 * p] = (uint8_t)v;
            out[3 * p + 1] = (uint8_t)(v >> 8);
            out[3 * p + 2] = (uint8_t)(v >> 16);
        }
    }
}

}  // namespace hmm

using namespace hmm;

namespace {
bool layout_of(const int32_t* geometry, int x0, int y0, int w, int h, JpegLayout* L) {
    return geometry && jpeg_layout(geometry[0], geometry[1], geometry[2], geometry[3], geometry[4], x0, y0, w, h, L);
}
}  // namespace

extern "C" size_t hmm_jpeg_workspace_bytes(const int32_t* geometry, int n, int x0, int y0, int w, int h) {
    JpegLayout L;
    if (n < 1 || !layout_of(geometry, x0, y0, w, h, &L)) return 0;
    return align_up((size_t)n * (size_t)L.plane_off[L.ncomp], 256);
}

extern "C" int hmm_jpeg_reconstruct(const void* slots_dev, int n, size_t slot_stride, const int32_t* geometry, int x0, int y0,
                                    int w, int h, uint8_t* rgb_out_dev, void* workspace_dev, size_t workspace_bytes,
                                    hmm_stream_t stream) {
    HMM_REQUIRE(slots_dev && geometry && rgb_out_dev && workspace_dev, HMM_E_INVALID, "jpeg_reconstruct: null pointer");
    JpegLayout L;
    HMM_REQUIRE(layout_of(geometry, x0, y0, w, h, &L), HMM_E_INVALID, "jpeg_reconstruct: bad geometry or window (%d, %d, %d, %d)",
                x0, y0, w, h);
    HMM_REQUIRE(n >= 1, HMM_E_INVALID, "jpeg_reconstruct: n = %d", n);
    HMM_REQUIRE(slot_stride >= (size_t)L.slot_bytes && slot_stride % 16 == 0, HMM_E_INVALID,
                "jpeg_reconstruct: slot stride %zu (>= %lld and a multiple of 16 needed)", slot_stride, (long long)L.slot_bytes);
    HMM_REQUIRE(((uintptr_t)slots_dev & 15) == 0 && ((uintptr_t)rgb_out_dev & 3) == 0 && ((uintptr_t)workspace_dev & 15) == 0,
                HMM_E_INVALID, "jpeg_reconstruct: slots and workspace must be 16-byte aligned, the output 4-byte aligned");
    HMM_REQUIRE(workspace_bytes >= hmm_jpeg_workspace_bytes(geometry, n, x0, y0, w, h), HMM_E_WORKSPACE,
                "jpeg_reconstruct: workspace of %zu bytes, %zu needed", workspace_bytes,
                hmm_jpeg_workspace_bytes(geometry, n, x0, y0, w, h));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t blocks = (int64_t)n * L.block_off[L.ncomp];
    const int64_t groups = (blocks + kIdctBlocks - 1) / kIdctBlocks;
    HMM_REQUIRE(groups <= 0x7FFFFFFF, HMM_E_INVALID, "jpeg_reconstruct: %lld blocks in one call is too many", (long long)blocks);
    jpeg_idct_kernel<<<(unsigned)groups, kIdctBlocks * 8, 0, st>>>(static_cast<const uint8_t*>(slots_dev), (int64_t)slot_stride, n, L,
                                                                   static_cast<uint8_t*>(workspace_dev));
    HMM_LAUNCH_CHECK();
    const int64_t quads = ((int64_t)n * w * h + 3) / 4;
    const int64_t color_groups = (quads + kColorThreads - 1) / kColorThreads;
    HMM_REQUIRE(color_groups <= 0x7FFFFFFF, HMM_E_INVALID, "jpeg_reconstruct: output too large for one call");
    jpeg_color_kernel<<<(unsigned)color_groups, kColorThreads, 0, st>>>(static_cast<const uint8_t*>(workspace_dev), L, n, rgb_out_dev);
    HMM_LAUNCH_CHECK();
    return HMM_OK;
}

// The window's planes are those of hmm_jpeg_reconstruct for the same geometry and window, so the workspace is too.
extern "C" size_t hmm_jpeg_encoded_pixels_workspace_bytes(const int32_t* geometry, int n, int x0, int y0, int w, int h) {
    JpegEncLayout E;
    if (!geometry || !jpeg_enc_layout(geometry[0], geometry[1], geometry[2], geometry[3], geometry[4], &E)) return 0;
    return hmm_jpeg_workspace_bytes(geometry, n, x0, y0, w, h);
}

extern "C" int hmm_jpeg_encoded_pixels(const void* encode_workspace_dev, int n, const int32_t* geometry, const uint16_t* qtables_dev,
                                       int x0, int y0, int w, int h, uint8_t* rgb_out_dev, void* workspace_dev,
                                       size_t workspace_bytes, hmm_stream_t stream) {
    HMM_REQUIRE(encode_workspace_dev && geometry && qtables_dev && rgb_out_dev && workspace_dev, HMM_E_INVALID,
                "jpeg_encoded_pixels: null pointer");
    HMM_REQUIRE(n >= 0, HMM_E_INVALID, "jpeg_encoded_pixels: negative frame count %d", n);
    JpegEncLayout E;
    HMM_REQUIRE(jpeg_enc_layout(geometry[0], geometry[1], geometry[2], geometry[3], geometry[4], &E), HMM_E_INVALID,
                "jpeg_encoded_pixels: bad geometry (%d x %d, %d components, sampling %d x %d): what hmm_jpeg_encode takes",
                geometry[0], geometry[1], geometry[2], geometry[3], geometry[4]);
    JpegLayout L;
    HMM_REQUIRE(layout_of(geometry, x0, y0, w, h, &L), HMM_E_INVALID, "jpeg_encoded_pixels: bad window (%d, %d, %d, %d) for a %d x %d frame",
                x0, y0, w, h, geometry[0], geometry[1]);
    HMM_REQUIRE(((uintptr_t)encode_workspace_dev & 15) == 0 && ((uintptr_t)workspace_dev & 15) == 0 && ((uintptr_t)rgb_out_dev & 3) == 0 &&
                    ((uintptr_t)qtables_dev & 1) == 0,
                HMM_E_INVALID, "jpeg_encoded_pixels: both workspaces must be 16-byte aligned, the output 4-byte and the tables 2-byte aligned");
    if (n == 0) return HMM_OK;
    const size_t need = hmm_jpeg_workspace_bytes(geometry, n, x0, y0, w, h);
    HMM_REQUIRE(workspace_bytes >= need, HMM_E_WORKSPACE, "jpeg_encoded_pixels: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t blocks = (int64_t)n * L.block_off[L.ncomp];
    const int64_t groups = (blocks + kIdctBlocks - 1) / kIdctBlocks;
    HMM_REQUIRE(groups <= 0x7FFFFFFF, HMM_E_INVALID, "jpeg_encoded_pixels: %lld blocks in one call is too many", (long long)blocks);
    const int64_t quads = ((int64_t)n * w * h + 3) / 4;
    const int64_t color_groups = (quads + kColorThreads - 1) / kColorThreads;
    HMM_REQUIRE(color_groups <= 0x7FFFFFFF, HMM_E_INVALID, "jpeg_encoded_pixels: output too large for one call");
    jpeg_encoded_idct_kernel<<<(unsigned)groups, kIdctBlocks * 8, 0, st>>>(static_cast<const int16_t*>(encode_workspace_dev), n, L, E,
                                                                           qtables_dev, static_cast<uint8_t*>(workspace_dev));
    HMM_LAUNCH_CHECK();
    jpeg_color_kernel<<<(unsigned)color_groups, kColorThreads, 0, st>>>(static_cast<const uint8_t*>(workspace_dev), L, n, rgb_out_dev);
    HMM_LAUNCH_CHECK();
    return HMM_OK;
}
