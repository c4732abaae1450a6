// The audio track of a video on the device: the kernels behind AudioTrack (hippomm_amd/audio_track.py).  Two replace the
// per-segment slice / mono / float32 / peak-normalise / wav round trip / resample / clip of the reference's process_sequence
// (hippomm/core/hippocampal_memory.py:1198-1251 and imagebind.data.load_and_transform_audio_data behind it); the third gives the
// audio-level scan of _segment_sequence (:993-1000, :1061-1077) its sums of squares.
//
//   peaks    span_peaks_kernel: one workgroup per span, max |x| over the NARROWED samples (fp64 -> fp32 round-to-nearest-even, the
//            bits of ndarray.astype(float32)).  The maximum is taken on the bit patterns of |x| as unsigned integers: for numbers
//            that is the order of the values, and every NaN pattern lies above infinity, so a NaN anywhere in the span is what
//            comes out -- np.abs(x).max() -- where an fmaxf reduction would drop it.  16-byte loads over the part of the span that
//            is 16-byte aligned (span starts are arbitrary sample indices), element loads for the head and the tail: no byte
//            outside [start, end) is read.
//   gather   gather_clips_kernel: grid over (clip, block of 256 output samples).  A sample of the span is narrowed and, when the
//            span's peak p > 1.0f, divided by p (one correctly rounded fp32 division; p == 1.0f and a NaN p leave it alone).
//            orig == new: that value is the output sample -- a copy, bit-exact.  Otherwise the span is resampled as a file of its
//            own: out[j] = sum_t taps[j % new][t] * x[(j / new) * orig - width + t] with x zero outside [0, span_len) -- samples
//            of the track outside the span never enter.  The workgroup stages the input window of its 256 outputs in LDS (already
//            narrowed and scaled); the tap table is tap-major, (T, new), so the lanes of a wave -- consecutive j, hence
//            consecutive phases -- read consecutive floats.  fp32 fused multiply-adds into four partial sums (t mod 4), added as
//            (a0 + a1) + (a2 + a3): one fixed order, so a clip's bits do not depend on the batch it rides in or on the run.
//
//   levels   window_sums_kernel: one workgroup per window, the sum of squares of its samples in the track's own dtype and in the
//            order of np.mean(np.square(x)) on a contiguous window (numpy 2.x: the ufunc buffer of 8192 elements, then
//            pairwise_sum), so that the dB level formed from it on the host carries the bits of the reference's audio level
//            (hippocampal_memory.py:993-1000).  Squares are a multiply rounded on its own (contraction is off from that kernel
//            on).  The window is cut into chunks of 8192 squares whose sums are added left to right.  A chunk of m squares is
//            numpy's split tree: m > 128 splits at (m / 2) - (m / 2) % 8.  The tree (depth <= 7) is expanded level by level into
//            a heap in LDS, node i with children 2i and 2i + 1.  A leaf (m <= 128) goes to eight lanes: lane j holds numpy's
//            accumulator r_j (elements 8i + j, in order, from element j), the eight are combined by a butterfly over XOR 1, 2, 4
//            -- ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) in every lane, addition being commutative -- and the m % 8 tail elements
//            are added one by one; with no full row of eight that is numpy's running sum from 0 for m < 8.  Inner nodes are then
//            added bottom-up, left + right.  Element loads (a window starts at any sample): the eight lanes of a leaf read 32 or
//            64 consecutive bytes, and no byte outside the window is read.  The order is a function of the window's length
//            alone: not of the grid, the batch or the run.
//
//   16-bit   a track may also hold the int16 samples x of the extracted WAV, with the values sf.read gives them, x / 32768
//            (hmm_audio_pcm16_gather_clips, hmm_audio_pcm16_window_sums; hmm_segment_walk_pcm16 in segment_walk.hip).  The gather
//            gets a third loader, (float)x * 2^-15, and no peaks; the sums get a kernel of their own without the tree.  Both give
//            the bits of the fp64 track of x / 32768.0: the arguments stand at gather_clips_kernel and pcm16_window_sums_kernel.
//
// All of them read their span / clip / window tables from the device and clamp what they find there to the track, so a device table
// that disagrees with the host copy the entry point has checked reads and writes less, never elsewhere.  No scratch, vector stores
// only.
#include "audio_levels.h"

namespace hmm {

typedef float at_f32x4 __attribute__((ext_vector_type(4)));
typedef double at_f64x2 __attribute__((ext_vector_type(2)));
typedef int16_t at_i16x8 __attribute__((ext_vector_type(8)));

constexpr int kClipBlock = 256;                                               // output samples (= threads) per workgroup of the gather
constexpr int kPcmCopyBlock = 8 * kClipBlock;                                 // ... of the copy from a 16-bit track: eight per thread

__device__ __forceinline__ uint32_t abs_bits(float x) { return __float_as_uint(x) & 0x7FFFFFFFu; }
__device__ __forceinline__ uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }
__device__ __forceinline__ float pcm16_float(int16_t x) { return (float)x * 0x1p-15f; }     // exact: sf.read's x / 32768, narrowed

// What a track holds: kF32 and kF64 are track_dtype 0 and 1 of the C ABI; kPcm16 is the layout of the hmm_audio_pcm16_* entry points.
constexpr int kF32 = 0, kF64 = 1, kPcm16 = 2;

template <int SRC>
__device__ __forceinline__ float load_narrow(const void* __restrict__ track, int64_t i) {
    if constexpr (SRC == kF64) return (float)static_cast<const double*>(track)[i];      // v_cvt_f32_f64: round to nearest even
    else if constexpr (SRC == kPcm16) return pcm16_float(static_cast<const int16_t*>(track)[i]);
    else return static_cast<const float*>(track)[i];
}

template <bool F64>
__device__ __forceinline__ uint32_t abs_bits16(const void* __restrict__ track, int64_t first, int64_t v) {
    if constexpr (F64) {
        const at_f64x2 d = reinterpret_cast<const at_f64x2*>(static_cast<const double*>(track) + first)[v];
        return umax(abs_bits((float)d[0]), abs_bits((float)d[1]));
    } else {
        const at_f32x4 f = reinterpret_cast<const at_f32x4*>(static_cast<const float*>(track) + first)[v];
        return umax(umax(abs_bits(f[0]), abs_bits(f[1])), umax(abs_bits(f[2]), abs_bits(f[3])));
    }
}

template <bool F64>
__global__ __launch_bounds__(256) void span_peaks_kernel(const void* __restrict__ track, int64_t track_len,
                                                         const int64_t* __restrict__ spans, float* __restrict__ peaks) {
    constexpr int V = F64 ? 2 : 4;                                            // elements per 16 bytes
    __shared__ uint32_t part[4];
    const int tid = threadIdx.x;
    int64_t a = spans[2 * blockIdx.x], b = spans[2 * blockIdx.x + 1];
    a = a < 0 ? 0 : (a > track_len ? track_len : a);
    b = b < a ? a : (b > track_len ? track_len : b);
    int64_t body = (a + V - 1) / V * V;                                       // the track is 16-byte aligned: so is element `body`
    if (body > b) body = b;
    const int64_t n_vec = (b - body) / V;
    uint32_t m = 0;
    for (int64_t i = a + tid; i < body; i += 256) m = umax(m, abs_bits(load_narrow<F64>(track, i)));
    int64_t v = tid;
    for (; v + 768 < n_vec; v += 1024) {                                      // four loads in flight per lane
        const uint32_t m0 = abs_bits16<F64>(track, body, v), m1 = abs_bits16<F64>(track, body, v + 256);
        const uint32_t m2 = abs_bits16<F64>(track, body, v + 512), m3 = abs_bits16<F64>(track, body, v + 768);
        m = umax(m, umax(umax(m0, m1), umax(m2, m3)));
    }
    for (; v < n_vec; v += 256) m = umax(m, abs_bits16<F64>(track, body, v));
    for (int64_t i = body + n_vec * V + tid; i < b; i += 256) m = umax(m, abs_bits(load_narrow<F64>(track, i)));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = umax(m, (uint32_t)__shfl_xor((int)m, off, 64));
    if ((tid & 63) == 0) part[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) peaks[blockIdx.x] = __uint_as_float(umax(umax(part[0], part[1]), umax(part[2], part[3])));
}

// clips: per clip (span start, span length, first output sample of the clip in the span's 16 kHz signal, span index).
// A 16-bit track (SRC == kPcm16) has no peaks: |x / 32768| <= 1 always (-32768 gives exactly 1.0, and 1.0f > 1.0f is false), so no
// span is ever scaled; peaks is null, the span index of a clip row is not looked at, and the samples are (float)x * 2^-15 -- exact,
// the float the fp64 track of x / 32768.0 narrows to -- so both instantiations give that track's bits.  Its copy case moves
// kPcmCopyBlock samples per workgroup: the 16-byte groups of eight samples that lie whole inside the block's part of the clip
// (the track is 16-byte aligned, a clip starts at any sample), elements before the first and behind the last of them, through
// LDS, from where the floats leave in order.  Nothing outside [start + first, start + first + clip_len) is read.
template <int SRC, bool RESAMPLE>
__global__ __launch_bounds__(kClipBlock) void gather_clips_kernel(const void* __restrict__ track, int64_t track_len,
                                                                  const int64_t* __restrict__ clips, const float* __restrict__ peaks,
                                                                  int n_spans, int clip_len, int blocks_per_clip, int orig, int new_,
                                                                  int width, const float* __restrict__ taps, float* __restrict__ out) {
    extern __shared__ float window[];
    constexpr bool PCM = SRC == kPcm16;
    const int tid = threadIdx.x;
    const int c = blockIdx.x / blocks_per_clip, i0 = (blockIdx.x % blocks_per_clip) * (PCM && !RESAMPLE ? kPcmCopyBlock : kClipBlock);
    int64_t start = clips[4 * c], len = clips[4 * c + 1];
    const int64_t first = clips[4 * c + 2], span = PCM ? 0 : clips[4 * c + 3];
    if (start < 0 || start > track_len || len < 0 || first < 0 || span < 0 || (!PCM && span >= n_spans)) return;   // workgroup-uniform
    if (len > track_len - start) len = track_len - start;
    float p = 0.0f;
    if constexpr (!PCM) p = peaks[span];
    const bool scale = p > 1.0f;                                              // false for p == 1 and for a NaN peak
    const int i = i0 + tid;                                                   // sample of the clip
    float* dst = out + (int64_t)c * clip_len;
    if constexpr (!RESAMPLE && PCM) {
        int64_t n = len - first;                                              // samples of the clip the span holds
        if (n > clip_len) n = clip_len;
        if (n <= i0) return;                                                  // workgroup-uniform
        const int i1 = i0 + (int)(n - i0 < kPcmCopyBlock ? n - i0 : kPcmCopyBlock);                 // this workgroup: clip samples [i0, i1)
        const int16_t* __restrict__ src = static_cast<const int16_t*>(track) + start + first;       // clip sample 0
        int head = i1 - i0 < 8 ? i1 : i0 + (int)((8 - ((start + first + i0) & 7)) & 7);             // the first clip sample at a 16-byte boundary
        if (head > i1) head = i1;
        const int n_vec = (i1 - head) >> 3;                                   // at most kPcmCopyBlock / 8 = one per thread
        const int tail = head + 8 * n_vec;
        if (i0 + tid < head) window[tid] = pcm16_float(src[i0 + tid]);
        if (tid < n_vec) {
            const at_i16x8 v = reinterpret_cast<const at_i16x8*>(src + head)[tid];
#pragma unroll
            for (int k = 0; k < 8; ++k) window[head - i0 + 8 * tid + k] = pcm16_float(v[k]);
        }
        if (tail + tid < i1) window[tail - i0 + tid] = pcm16_float(src[tail + tid]);
        __syncthreads();
        for (int k = tid; k < i1 - i0; k += kClipBlock) dst[i0 + k] = window[k];
    } else if constexpr (!RESAMPLE) {
        if (i < clip_len && first + i < len) {
            const float x = load_narrow<SRC>(track, start + first + i);
            dst[i] = scale ? __fdiv_rn(x, p) : x;
        }
    } else {
        const int taps_n = 2 * width + orig;
        const int last = (i0 + kClipBlock <= clip_len ? i0 + kClipBlock : clip_len) - 1;
        const int64_t f0 = (first + i0) / new_, f1 = (first + last) / new_;  // input frames of the block's first / last output
        const int64_t x0 = f0 * orig - width;
        const int n_win = (int)(f1 - f0) * orig + taps_n;
        for (int k = tid; k < n_win; k += kClipBlock) {
            const int64_t xi = x0 + k;
            float x = 0.0f;                                                   // outside the span: zero, whatever the track holds there
            if (xi >= 0 && xi < len) {
                x = load_narrow<SRC>(track, start + xi);
                if (scale) x = __fdiv_rn(x, p);
            }
            window[k] = x;
        }
        __syncthreads();
        const int64_t n_out = (len * new_ + orig - 1) / orig;
        if (i < clip_len && first + i < n_out) {
            const int64_t j = first + i;
            const float* __restrict__ tp = taps + (int)(j % new_);
            const float* xp = window + (int)(j / new_ - f0) * orig;
            float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
            int t = 0;
            for (; t + 4 <= taps_n; t += 4) {
                a0 = __fmaf_rn(tp[(int64_t)t * new_], xp[t], a0);
                a1 = __fmaf_rn(tp[(int64_t)(t + 1) * new_], xp[t + 1], a1);
                a2 = __fmaf_rn(tp[(int64_t)(t + 2) * new_], xp[t + 2], a2);
                a3 = __fmaf_rn(tp[(int64_t)(t + 3) * new_], xp[t + 3], a3);
            }
            if (t < taps_n) a0 = __fmaf_rn(tp[(int64_t)t * new_], xp[t], a0);
            if (t + 1 < taps_n) a1 = __fmaf_rn(tp[(int64_t)(t + 1) * new_], xp[t + 1], a1);
            if (t + 2 < taps_n) a2 = __fmaf_rn(tp[(int64_t)(t + 2) * new_], xp[t + 2], a2);
            dst[i] = (a0 + a1) + (a2 + a3);
        }
    }
}

// ---- window sums: everything from here on is compiled with contraction off (x * x + r must stay a multiply and an add) ----------
#pragma clang fp contract(off)

constexpr int kSumChunk = 8192;                                               // numpy's ufunc buffer, in elements
constexpr int kSumLeaf = 128;                                                 // pairwise_sum's PW_BLOCKSIZE
constexpr int kSumNodes = 256;                                                // heap ids 1 .. 255: depth 7 is the deepest a chunk reaches
constexpr int kSumDepth = 7;

// The sum of squares of one leaf, s[0 .. len), by the eight lanes j = 0 .. 7 of a group; every lane returns it.  len == 0 (no leaf
// for this group) reads nothing.  All lanes of the wave execute the shuffles.
template <typename T>
__device__ __forceinline__ T leaf_sum_squares(const T* __restrict__ s, int len, int j) {
    const int rows = len >> 3;                                                // full rows of eight: at most 16
    T x[kSumLeaf / 8];
#pragma unroll
    for (int i = 0; i < kSumLeaf / 8; ++i) x[i] = i < rows ? s[8 * i + j] : T(0);
    T r = x[0] * x[0];
#pragma unroll
    for (int i = 1; i < kSumLeaf / 8; ++i)
        if (i < rows) r = r + x[i] * x[i];
    r = r + __shfl_xor(r, 1, 64);
    r = r + __shfl_xor(r, 2, 64);
    r = r + __shfl_xor(r, 4, 64);
    for (int i = rows * 8; i < len; ++i) {                                    // the tail, or all of a leaf shorter than 8
        const T t = s[i];
        r = r + t * t;
    }
    return r;
}

template <typename T>
__global__ __launch_bounds__(256) void window_sums_kernel(const T* __restrict__ track, int64_t track_len,
                                                          const int64_t* __restrict__ windows, T* __restrict__ sums) {
    __shared__ int node_off[kSumNodes], node_len[kSumNodes];
    __shared__ T node_sum[kSumNodes];
    const int tid = threadIdx.x, group = tid >> 3, j = tid & 7;
    int64_t start = windows[2 * blockIdx.x], n = windows[2 * blockIdx.x + 1];
    start = start < 0 ? 0 : (start > track_len ? track_len : start);
    n = n < 0 ? 0 : (n > track_len - start ? track_len - start : n);
    const T* __restrict__ win = track + start;
    T total = T(0);
    int expanded = -1;                                                        // the chunk length the heap in LDS was expanded for
    for (int64_t c0 = 0; c0 < n; c0 += kSumChunk) {                           // workgroup-uniform
        const int m = (int)(n - c0 < kSumChunk ? n - c0 : kSumChunk);
        if (m != expanded) {
            if (tid < 2) {
                node_off[tid] = 0;
                node_len[tid] = tid == 1 ? m : 0;
            }
            __syncthreads();
            for (int d = 0; d < kSumDepth; ++d) {
                if (tid >= (1 << d) && tid < (2 << d)) {
                    const int len = node_len[tid], off = node_off[tid];
                    const int half = len >> 1, left = len > kSumLeaf ? half - (half & 7) : 0;
                    node_off[2 * tid] = off;
                    node_len[2 * tid] = left;
                    node_off[2 * tid + 1] = off + left;
                    node_len[2 * tid + 1] = len > kSumLeaf ? len - left : 0;
                }
                __syncthreads();
            }
            expanded = m;
        }
        for (int node = group; node < kSumNodes; node += 32) {                // leaves: one per group of eight lanes
            int len = node_len[node];
            if (len > kSumLeaf) len = 0;                                      // an inner node
            if (__ballot(len > 0) == 0) continue;                             // wave-uniform
            const T r = leaf_sum_squares<T>(win + c0 + node_off[node], len, j);
            if (len > 0 && j == 0) node_sum[node] = r;
        }
        __syncthreads();
        for (int d = kSumDepth - 1; d >= 0; --d) {                            // inner nodes, bottom-up: left + right
            if (tid >= (1 << d) && tid < (2 << d) && node_len[tid] > kSumLeaf) node_sum[tid] = node_sum[2 * tid] + node_sum[2 * tid + 1];
            __syncthreads();
        }
        total = total + node_sum[1];                                          // chunk sums left to right, the same in every thread
        __syncthreads();                                                      // node_sum is free for the next chunk
    }
    if (tid == 0) sums[blockIdx.x] = total;
}

void launch_window_sums(const void* track_dev, int track_dtype, int64_t track_len, const int64_t* windows_dev, int n_windows,
                        void* sums_dev, hipStream_t stream) {
    if (track_dtype == 1)
        window_sums_kernel<double><<<n_windows, 256, 0, stream>>>(static_cast<const double*>(track_dev), track_len, windows_dev,
                                                                   static_cast<double*>(sums_dev));
    else
        window_sums_kernel<float><<<n_windows, 256, 0, stream>>>(static_cast<const float*>(track_dev), track_len, windows_dev,
                                                                  static_cast<float*>(sums_dev));
}

// The sums of a 16-bit track: sums[w] = the fp64 sum of (x / 32768)^2 over the window, the bits window_sums_kernel<double> gives on
// the fp64 track of x / 32768.0 -- without its tree.  Why any order will do: x / 32768 is exact in fp64, and its square is the
// integer x^2 <= 2^30 times 2^-30, exact as well.  Over a window of at most kPcmWindowMax = 2^22 samples every partial sum of such
// squares, in any order, is an integer <= 2^52 times 2^-30: exactly representable, so no addition of numpy's pairwise sum ever
// rounds, and its result is the exact sum.  Here that sum is taken in integers -- two squares fit 32 bits unsigned, the rest is
// 64-bit -- and scaled by 2^-30 once: one rounding-free conversion.  One workgroup per window: 16-byte loads of eight samples over
// the part of the window that is 16-byte aligned, element loads for the head and the tail (no byte outside the window is read), a
// butterfly over the wave, four wave sums through LDS, one vector store.  A device table is clamped to the track and to 2^22.
__device__ __forceinline__ uint64_t squares8(const int16_t* __restrict__ body, int64_t v) {
    const at_i16x8 x = reinterpret_cast<const at_i16x8*>(body)[v];
    uint64_t s = 0;
#pragma unroll
    for (int k = 0; k < 8; k += 2) {
        const int32_t a = x[k], b = x[k + 1];
        s += (uint32_t)(a * a) + (uint32_t)(b * b);                           // at most 2^31: no carry is lost
    }
    return s;
}

__global__ __launch_bounds__(256) void pcm16_window_sums_kernel(const int16_t* __restrict__ track, int64_t track_len,
                                                                const int64_t* __restrict__ windows, double* __restrict__ sums) {
    __shared__ uint64_t part[4];
    const int tid = threadIdx.x;
    int64_t a = windows[2 * blockIdx.x], n = windows[2 * blockIdx.x + 1];
    a = a < 0 ? 0 : (a > track_len ? track_len : a);
    n = n < 0 ? 0 : (n > track_len - a ? track_len - a : n);
    if (n > kPcmWindowMax) n = kPcmWindowMax;
    const int64_t b = a + n;
    int64_t body = (a + 7) / 8 * 8;                                           // the track is 16-byte aligned: so is element `body`
    if (body > b) body = b;
    const int64_t n_vec = (b - body) / 8;
    uint64_t s = 0;
    for (int64_t i = a + tid; i < body; i += 256) {
        const int32_t x = track[i];
        s += (uint32_t)(x * x);
    }
    int64_t v = tid;
    for (; v + 768 < n_vec; v += 1024) {                                      // four loads in flight per lane
        const uint64_t s0 = squares8(track + body, v), s1 = squares8(track + body, v + 256);
        const uint64_t s2 = squares8(track + body, v + 512), s3 = squares8(track + body, v + 768);
        s += (s0 + s1) + (s2 + s3);
    }
    for (; v < n_vec; v += 256) s += squares8(track + body, v);
    for (int64_t i = body + n_vec * 8 + tid; i < b; i += 256) {
        const int32_t x = track[i];
        s += (uint32_t)(x * x);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)s, off, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(s >> 32), off, 64);
        s += ((uint64_t)hi << 32) | lo;
    }
    if ((tid & 63) == 0) part[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) sums[blockIdx.x] = (double)((part[0] + part[1]) + (part[2] + part[3])) * 0x1p-30;
}

void launch_pcm16_window_sums(const void* track_dev, int64_t track_len, const int64_t* windows_dev, int n_windows, double* sums_dev,
                              hipStream_t stream) {
    pcm16_window_sums_kernel<<<n_windows, 256, 0, stream>>>(static_cast<const int16_t*>(track_dev), track_len, windows_dev, sums_dev);
}

static bool track_overlap(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes) {
    const uint64_t x = (uint64_t)(uintptr_t)a, y = (uint64_t)(uintptr_t)b;
    return a_bytes != 0 && b_bytes != 0 && x < y + b_bytes && y < x + a_bytes;
}

}  // namespace hmm

using namespace hmm;

extern "C" int hmm_audio_span_peaks(const void* track_dev, int track_dtype, int64_t track_len, const int64_t* spans_host,
                                    const int64_t* spans_dev, int n_spans, float* peaks_out_dev, hmm_stream_t stream) {
    HMM_REQUIRE(track_dtype == 0 || track_dtype == 1, HMM_E_INVALID, "audio_span_peaks: track_dtype must be 0 (fp32) or 1 (fp64), got %d",
                track_dtype);
    HMM_REQUIRE(track_len >= 0 && n_spans >= 0, HMM_E_INVALID, "audio_span_peaks: negative count (track_len=%lld, n_spans=%d)",
                (long long)track_len, n_spans);
    if (n_spans == 0) return HMM_OK;                                          // nothing to write: no pointer is looked at
    HMM_REQUIRE(track_dev && spans_host && spans_dev && peaks_out_dev, HMM_E_INVALID, "audio_span_peaks: null pointer");
    HMM_REQUIRE(((uintptr_t)track_dev & 15) == 0 && ((uintptr_t)spans_dev & 7) == 0 && ((uintptr_t)peaks_out_dev & 3) == 0, HMM_E_INVALID,
                "audio_span_peaks: the track must be 16-byte aligned, the tables aligned to their element size");
    for (int s = 0; s < n_spans; ++s) {
        const int64_t a = spans_host[2 * s], b = spans_host[2 * s + 1];
        HMM_REQUIRE(a >= 0 && a <= b && b <= track_len, HMM_E_INVALID,
                    "audio_span_peaks: span %d = [%lld, %lld) lies outside the track [0, %lld]", s, (long long)a, (long long)b,
                    (long long)track_len);
    }
    HMM_REQUIRE(!track_overlap(track_dev, (uint64_t)track_len * (track_dtype == 1 ? 8 : 4), peaks_out_dev, (uint64_t)n_spans * 4),
                HMM_E_INVALID, "audio_span_peaks: the output overlaps the track");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (track_dtype == 1) span_peaks_kernel<true><<<n_spans, 256, 0, st>>>(track_dev, track_len, spans_dev, peaks_out_dev);
    else span_peaks_kernel<false><<<n_spans, 256, 0, st>>>(track_dev, track_len, spans_dev, peaks_out_dev);
    HMM_LAUNCH_CHECK();
    return HMM_OK;
}

extern "C" int hmm_audio_gather_clips(const void* track_dev, int track_dtype, int64_t track_len, const int64_t* clips_host,
                                      const int64_t* clips_dev, int n_clips, const float* peaks_dev, int n_spans, int clip_len,
                                      int orig, int new_, int width, const float* taps_dev, float* clips_out_dev,
                                      hmm_stream_t stream) {
    HMM_REQUIRE(track_dtype == 0 || track_dtype == 1, HMM_E_INVALID, "audio_gather_clips: track_dtype must be 0 (fp32) or 1 (fp64), got %d",
                track_dtype);
    HMM_REQUIRE(track_len >= 0 && n_clips >= 0 && n_spans >= 0 && clip_len >= 0 && width >= 0, HMM_E_INVALID,
                "audio_gather_clips: negative count (track_len=%lld, n_clips=%d, n_spans=%d, clip_len=%d, width=%d)",
                (long long)track_len, n_clips, n_spans, clip_len, width);
    HMM_REQUIRE(orig >= 1 && new_ >= 1, HMM_E_INVALID, "audio_gather_clips: orig and new must be at least 1, got %d and %d", orig, new_);
    if (n_clips == 0 || clip_len == 0) return HMM_OK;                         // nothing to write: no pointer is looked at
    HMM_REQUIRE(track_dev && clips_host && clips_dev && peaks_dev && clips_out_dev, HMM_E_INVALID, "audio_gather_clips: null pointer");
    HMM_REQUIRE(orig == new_ || taps_dev != nullptr, HMM_E_INVALID,
                "audio_gather_clips: taps must be given when orig != new (%d -> %d): null pointer", orig, new_);
    HMM_REQUIRE(((uintptr_t)track_dev & 15) == 0 && ((uintptr_t)clips_dev & 7) == 0 && ((uintptr_t)peaks_dev & 3) == 0 &&
                    ((uintptr_t)taps_dev & 3) == 0 && ((uintptr_t)clips_out_dev & 3) == 0, HMM_E_INVALID,
                "audio_gather_clips: the track must be 16-byte aligned, tables and clips aligned to their element size");
    // the input window of one workgroup: the frames its 256 outputs start in, plus one filter length
    const int64_t win = orig == new_ ? 0 : ((int64_t)((kClipBlock - 1) / new_ + 1) * orig + 2 * (int64_t)width + orig);
    HMM_REQUIRE(win * 4 <= 65536, HMM_E_INVALID,
                "audio_gather_clips: resampling %d -> %d with width %d needs a window of %lld samples per workgroup, 16384 fit", orig,
                new_, width, (long long)win);
    for (int c = 0; c < n_clips; ++c) {
        const int64_t a = clips_host[4 * c], len = clips_host[4 * c + 1], first = clips_host[4 * c + 2], span = clips_host[4 * c + 3];
        HMM_REQUIRE(a >= 0 && len >= 0 && a <= track_len && len <= track_len - a, HMM_E_INVALID,
                    "audio_gather_clips: clip %d: span [%lld, %lld + %lld) lies outside the track [0, %lld]", c, (long long)a,
                    (long long)a, (long long)len, (long long)track_len);
        HMM_REQUIRE(span >= 0 && span < n_spans, HMM_E_INVALID, "audio_gather_clips: clip %d: span index %lld is not in [0, %d)", c,
                    (long long)span, n_spans);
        const int64_t n_out = orig == new_ ? len : (len / orig * new_ + (len % orig * new_ + orig - 1) / orig);      // ceil(new len / orig)
        HMM_REQUIRE(first >= 0 && first <= n_out && clip_len <= n_out - first, HMM_E_INVALID,
                    "audio_gather_clips: clip %d: samples [%lld, %lld + %d) reach past the span's output length %lld", c,
                    (long long)first, (long long)first, clip_len, (long long)n_out);
    }
    HMM_REQUIRE(!track_overlap(track_dev, (uint64_t)track_len * (track_dtype == 1 ? 8 : 4), clips_out_dev,
                               (uint64_t)n_clips * (uint64_t)clip_len * 4),
                HMM_E_INVALID, "audio_gather_clips: the output overlaps the track");
    const int blocks_per_clip = (clip_len + kClipBlock - 1) / kClipBlock;
    HMM_REQUIRE((int64_t)blocks_per_clip * n_clips <= 0x7FFFFFFF, HMM_E_INVALID,
                "audio_gather_clips: %d clips of %d samples exceed one launch", n_clips, clip_len);
    const unsigned grid = (unsigned)(blocks_per_clip * n_clips);
    const size_t lds = (size_t)win * 4;
    hipStream_t st = static_cast<hipStream_t>(stream);
#define HMM_GATHER(SRC, RS)                                                                                                          \
    gather_clips_kernel<SRC, RS><<<grid, kClipBlock, lds, st>>>(track_dev, track_len, clips_dev, peaks_dev, n_spans, clip_len,       \
                                                                blocks_per_clip, orig, new_, width, taps_dev, clips_out_dev)
    if (orig == new_) {
        if (track_dtype == 1) HMM_GATHER(kF64, false); else HMM_GATHER(kF32, false);
    } else {
        if (track_dtype == 1) HMM_GATHER(kF64, true); else HMM_GATHER(kF32, true);
    }
#undef HMM_GATHER
    HMM_LAUNCH_CHECK();
    return HMM_OK;
}

extern "C" int hmm_audio_pcm16_gather_clips(const void* track_dev, int64_t track_len, const int64_t* clips_host, const int64_t* clips_dev,
                                            int n_clips, int clip_len, int orig, int new_, int width, const float* taps_dev,
                                            float* clips_out_dev, hmm_stream_t stream) {
    HMM_REQUIRE(track_len >= 0 && n_clips >= 0 && clip_len >= 0 && width >= 0, HMM_E_INVALID,
                "audio_pcm16_gather_clips: negative count (track_len=%lld, n_clips=%d, clip_len=%d, width=%d)", (long long)track_len,
                n_clips, clip_len, width);
    HMM_REQUIRE(orig >= 1 && new_ >= 1, HMM_E_INVALID, "audio_pcm16_gather_clips: orig and new must be at least 1, got %d and %d", orig,
                new_);
    if (n_clips == 0 || clip_len == 0) return HMM_OK;                         // nothing to write: no pointer is looked at
    HMM_REQUIRE(track_dev && clips_host && clips_dev && clips_out_dev, HMM_E_INVALID, "audio_pcm16_gather_clips: null pointer");
    HMM_REQUIRE(orig == new_ || taps_dev != nullptr, HMM_E_INVALID,
                "audio_pcm16_gather_clips: taps must be given when orig != new (%d -> %d): null pointer", orig, new_);
    HMM_REQUIRE(((uintptr_t)track_dev & 15) == 0 && ((uintptr_t)clips_dev & 7) == 0 && ((uintptr_t)taps_dev & 3) == 0 &&
                    ((uintptr_t)clips_out_dev & 3) == 0, HMM_E_INVALID,
                "audio_pcm16_gather_clips: the track must be 16-byte aligned, table, taps and clips aligned to their element size");
    const int64_t win = orig == new_ ? kPcmCopyBlock : ((int64_t)((kClipBlock - 1) / new_ + 1) * orig + 2 * (int64_t)width + orig);
    HMM_REQUIRE(win * 4 <= 65536, HMM_E_INVALID,
                "audio_pcm16_gather_clips: resampling %d -> %d with width %d needs a window of %lld samples per workgroup, 16384 fit",
                orig, new_, width, (long long)win);
    for (int c = 0; c < n_clips; ++c) {
        const int64_t a = clips_host[4 * c], len = clips_host[4 * c + 1], first = clips_host[4 * c + 2];
        HMM_REQUIRE(a >= 0 && len >= 0 && a <= track_len && len <= track_len - a, HMM_E_INVALID,
                    "audio_pcm16_gather_clips: clip %d: span [%lld, %lld + %lld) lies outside the track [0, %lld]", c, (long long)a,
                    (long long)a, (long long)len, (long long)track_len);
        const int64_t n_out = orig == new_ ? len : (len / orig * new_ + (len % orig * new_ + orig - 1) / orig);      // ceil(new len / orig)
        HMM_REQUIRE(first >= 0 && first <= n_out && clip_len <= n_out - first, HMM_E_INVALID,
                    "audio_pcm16_gather_clips: clip %d: samples [%lld, %lld + %d) reach past the span's output length %lld", c,
                    (long long)first, (long long)first, clip_len, (long long)n_out);
    }
    HMM_REQUIRE(!track_overlap(track_dev, (uint64_t)track_len * 2, clips_out_dev, (uint64_t)n_clips * (uint64_t)clip_len * 4),
                HMM_E_INVALID, "audio_pcm16_gather_clips: the output overlaps the track");
    const int per_block = orig == new_ ? kPcmCopyBlock : kClipBlock;
    const int blocks_per_clip = (int)(((int64_t)clip_len + per_block - 1) / per_block);
    HMM_REQUIRE((int64_t)blocks_per_clip * n_clips <= 0x7FFFFFFF, HMM_E_INVALID,
                "audio_pcm16_gather_clips: %d clips of %d samples exceed one launch", n_clips, clip_len);
    const unsigned grid = (unsigned)(blocks_per_clip * n_clips);
    const size_t lds = (size_t)win * 4;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (orig == new_)
        gather_clips_kernel<kPcm16, false><<<grid, kClipBlock, lds, st>>>(track_dev, track_len, clips_dev, nullptr, 0, clip_len,
                                                                           blocks_per_clip, orig, new_, width, taps_dev, clips_out_dev);
    else
        gather_clips_kernel<kPcm16, true><<<grid, kClipBlock, lds, st>>>(track_dev, track_len, clips_dev, nullptr, 0, clip_len,
                                                                          blocks_per_clip, orig, new_, width, taps_dev, clips_out_dev);
    HMM_LAUNCH_CHECK();
    return HMM_OK;
}

extern "C" int hmm_audio_pcm16_window_sums(const void* track_dev, int64_t track_len, const int64_t* windows_host,
                                           const int64_t* windows_dev, int n_windows, double* sums_out_dev, hmm_stream_t stream) {
    HMM_REQUIRE(track_len >= 0 && n_windows >= 0, HMM_E_INVALID, "audio_pcm16_window_sums: negative count (track_len=%lld, n_windows=%d)",
                (long long)track_len, n_windows);
    if (n_windows == 0) return HMM_OK;                                        // nothing to write: no pointer is looked at
    HMM_REQUIRE(track_dev && windows_host && windows_dev && sums_out_dev, HMM_E_INVALID, "audio_pcm16_window_sums: null pointer");
    HMM_REQUIRE(((uintptr_t)track_dev & 15) == 0 && ((uintptr_t)windows_dev & 7) == 0 && ((uintptr_t)sums_out_dev & 7) == 0, HMM_E_INVALID,
                "audio_pcm16_window_sums: the track must be 16-byte aligned, the table and the sums aligned to their element size");
    for (int w = 0; w < n_windows; ++w) {
        const int64_t a = windows_host[2 * w], len = windows_host[2 * w + 1];
        HMM_REQUIRE(a >= 0 && len >= 0 && a <= track_len && len <= track_len - a, HMM_E_INVALID,
                    "audio_pcm16_window_sums: window %d = [%lld, %lld + %lld) lies outside the track [0, %lld]", w, (long long)a,
                    (long long)a, (long long)len, (long long)track_len);
        HMM_REQUIRE(len <= kPcmWindowMax, HMM_E_INVALID,
                    "audio_pcm16_window_sums: window %d is %lld samples long, above 4194304 (2^22) the sum is no longer exact", w,
                    (long long)len);
    }
    HMM_REQUIRE(!track_overlap(track_dev, (uint64_t)track_len * 2, sums_out_dev, (uint64_t)n_windows * 8), HMM_E_INVALID,
                "audio_pcm16_window_sums: the output overlaps the track");
    launch_pcm16_window_sums(track_dev, track_len, windows_dev, n_windows, sums_out_dev, static_cast<hipStream_t>(stream));
    HMM_LAUNCH_CHECK();
    return HMM_OK;
}

extern "C" int hmm_audio_window_sums(const void* track_dev, int track_dtype, int64_t track_len, const int64_t* windows_host,
                                     const int64_t* windows_dev, int n_windows, void* sums_out_dev, hmm_stream_t stream) {
    HMM_REQUIRE(track_dtype == 0 || track_dtype == 1, HMM_E_INVALID, "audio_window_sums: track_dtype must be 0 (fp32) or 1 (fp64), got %d",
                track_dtype);
    HMM_REQUIRE(track_len >= 0 && n_windows >= 0, HMM_E_INVALID, "audio_window_sums: negative count (track_len=%lld, n_windows=%d)",
                (long long)track_len, n_windows);
    if (n_windows == 0) return HMM_OK;                                        // nothing to write: no pointer is looked at
    HMM_REQUIRE(track_dev && windows_host && windows_dev && sums_out_dev, HMM_E_INVALID, "audio_window_sums: null pointer");
    const uint64_t elem = track_dtype == 1 ? 8 : 4;
    HMM_REQUIRE(((uintptr_t)track_dev & 15) == 0 && ((uintptr_t)windows_dev & 7) == 0 && ((uintptr_t)sums_out_dev & (elem - 1)) == 0,
                HMM_E_INVALID, "audio_window_sums: the track must be 16-byte aligned, the table and the sums aligned to their element size");
    for (int w = 0; w < n_windows; ++w) {
        const int64_t a = windows_host[2 * w], len = windows_host[2 * w + 1];
        HMM_REQUIRE(a >= 0 && len >= 0 && a <= track_len && len <= track_len - a, HMM_E_INVALID,
                    "audio_window_sums: window %d = [%lld, %lld + %lld) lies outside the track [0, %lld]", w, (long long)a, (long long)a,
                    (long long)len, (long long)track_len);
    }
    HMM_REQUIRE(!track_overlap(track_dev, (uint64_t)track_len * elem, sums_out_dev, (uint64_t)n_windows * elem), HMM_E_INVALID,
                "audio_window_sums: the output overlaps the track");
    launch_window_sums(track_dev, track_dtype, track_len, windows_dev, n_windows, sums_out_dev, static_cast<hipStream_t>(stream));
    HMM_LAUNCH_CHECK();
    return HMM_OK;
}
