// Base64 on the device, for the checkpoint file (hippomm/core/hippocampal_memory.py:1486-1524): a feature block is written there as
// base64(np.array(v.tolist()).tobytes()), i.e. the fp32 block widened to float64 and encoded.
//
// Encode: the output length is known in advance (4 * ceil(bytes / 3)), so this is ONE launch -- no scan, no workspace, no count to
// read back.  A thread takes one group of base64_core.h: 24 source bytes (three doubles; for an fp32 source three floats, widened
// here) -> 32 characters, stored as two 16-byte pieces.  Only the text's last group can be partial; it goes out as 4-byte quads, the
// last of them padded.  A wave reads 64 x 24 consecutive bytes and writes 64 x 32 consecutive characters.
//
// Decode is strict and leaves `out` untouched when it refuses, so it takes three launches on the caller's stream:
//   1. b64_report_init:  the report's words get their start values;
//   2. b64_check_kernel: every quad against the rules of check_quad; the lowest offending offset wins through one 64-bit atomicMin
//                        per offending thread; the thread that owns the last quad also counts the values;
//   3. b64_decode_kernel: nothing but the report if step 2 found something; else 32 characters -> 24 bytes per thread, stored as
//                        doubles, as narrowed floats (with the count of the ones that do not widen back) or as bytes.
// No allocation, no synchronisation, no LDS, no scratch, no wait between workgroups.
#include "hmm_common.h"
#include "base64_core.h"

namespace {

using namespace hmm;
using namespace hmm_b64;

constexpr int kThreads = HMM_BASE64_THREADS_PER_GROUP;
static_assert(HMM_BASE64_BYTES_PER_GROUP == kThreads * kGroupBytes, "the header states the workgroup's unit");
static_assert(HMM_BASE64_DTYPE_F32 == HMM_JSON_DTYPE_F32 && HMM_BASE64_DTYPE_F64 == HMM_JSON_DTYPE_F64, "one numbering of the float dtypes");

enum { R_STATUS = 0, R_OFFSET = 1, R_INEXACT = 2, R_VALUES = 3, R_KEY = 4 };
static_assert(HMM_BASE64_REPORT_WORDS == 5, "status, offset, inexact, values, key");

// ---- encode ----------------------------------------------------------------------------------------------------------------
// The three words of group g; values behind n_values read as zero.  DT: HMM_BASE64_DTYPE_*.
template <int DT>
__device__ __forceinline__ void load_group(const void* __restrict__ src, uint64_t g, uint64_t n_values, uint64_t w[3]) {
    if constexpr (DT == HMM_BASE64_DTYPE_F64) {
        const uint64_t* p = static_cast<const uint64_t*>(src);
#pragma unroll
        for (int k = 0; k < 3; ++k) w[k] = g * 3 + k < n_values ? p[g * 3 + k] : 0;
    } else if constexpr (DT == HMM_BASE64_DTYPE_F32) {
        const float* p = static_cast<const float*>(src);
#pragma unroll
        for (int k = 0; k < 3; ++k) w[k] = g * 3 + k < n_values ? bits_of((double)p[g * 3 + k]) : 0;   // what np.array(v.tolist()) holds
    } else {
        const uint8_t* p = static_cast<const uint8_t*>(src);
        w[0] = w[1] = w[2] = 0;
#pragma unroll
        for (int i = 0; i < kGroupBytes; ++i)
            if (g * kGroupBytes + i < n_values) w[i >> 3] |= (uint64_t)p[g * kGroupBytes + i] << (8 * (i & 7));
    }
}

template <int DT>
__global__ __launch_bounds__(kThreads) void b64_encode_kernel(const void* __restrict__ src, uint64_t n_values, uint64_t n_bytes,
                                                              char* __restrict__ out) {
    const uint64_t g = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (g * kGroupBytes >= n_bytes) return;
    const uint64_t left = n_bytes - g * kGroupBytes;
    const uint32_t here = left < (uint64_t)kGroupBytes ? (uint32_t)left : (uint32_t)kGroupBytes;
    uint64_t w[3];
    load_group<DT>(src, g, n_values, w);
    uint32_t quads[kGroupQuads];
    encode_group(w, here, quads);
    if (here == (uint32_t)kGroupBytes) {
        uint4* o = reinterpret_cast<uint4*>(out + g * kGroupChars);                  // out is 16-byte aligned, a group is 32 bytes
        o[0] = make_uint4(quads[0], quads[1], quads[2], quads[3]);
        o[1] = make_uint4(quads[4], quads[5], quads[6], quads[7]);
    } else {
        uint32_t* o = reinterpret_cast<uint32_t*>(out + g * kGroupChars);
        const uint32_t n_quads = (here + 2) / 3;
#pragma unroll
        for (int q = 0; q < kGroupQuads; ++q)
            if ((uint32_t)q < n_quads) o[q] = quads[q];
    }
}

// ---- decode ----------------------------------------------------------------------------------------------------------------
__global__ void b64_report_init(uint64_t* __restrict__ report, uint64_t status, uint64_t offset, uint64_t key) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        report[R_STATUS] = status;
        report[R_OFFSET] = offset;
        report[R_INEXACT] = 0;
        report[R_VALUES] = 0;
        report[R_KEY] = key;
    }
}

// The quads of group g (n_quads in the whole text; quads behind the text read as "AAAA", which decodes as zero bytes).
__device__ __forceinline__ void load_quads(const char* __restrict__ text, uint64_t g, uint64_t n_quads, uint32_t quads[kGroupQuads]) {
    if ((g + 1) * kGroupQuads <= n_quads) {
        const uint4* p = reinterpret_cast<const uint4*>(text + g * kGroupChars);      // text is 16-byte aligned
        const uint4 a = p[0], b = p[1];
        quads[0] = a.x; quads[1] = a.y; quads[2] = a.z; quads[3] = a.w;
        quads[4] = b.x; quads[5] = b.y; quads[6] = b.z; quads[7] = b.w;
    } else {
        const uint32_t* p = reinterpret_cast<const uint32_t*>(text + g * kGroupChars);
#pragma unroll
        for (int q = 0; q < kGroupQuads; ++q) quads[q] = g * kGroupQuads + q < n_quads ? p[q] : 0x41414141u;
    }
}

__global__ __launch_bounds__(kThreads) void b64_check_kernel(const char* __restrict__ text, uint64_t n_quads, int dtype, uint64_t cap_values,
                                                             uint64_t* __restrict__ report) {
    const uint64_t g = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (g * kGroupQuads >= n_quads) return;
    uint32_t quads[kGroupQuads];
    load_quads(text, g, n_quads, quads);
    uint64_t key = kNoKey;
#pragma unroll
    for (int q = 0; q < kGroupQuads; ++q) {
        const uint64_t Q = g * kGroupQuads + q;
        if (Q < n_quads) {
            uint32_t pad;
            const bool last = Q + 1 == n_quads;
            uint64_t k = check_quad(quads[q], Q * 4, last, &pad);
            if (last && k == kNoKey) {
                uint64_t n_values;
                const uint32_t status = count_values(n_quads, pad, dtype, cap_values, &n_values);
                if (status != HMM_BASE64_OK) k = key_of(Q * 4, status);
                else report[R_VALUES] = n_values;
            }
            key = k < key ? k : key;
        }
    }
    if (key != kNoKey) atomicMin(reinterpret_cast<unsigned long long*>(report + R_KEY), (unsigned long long)key);
}

template <int DT>
__global__ __launch_bounds__(kThreads) void b64_decode_kernel(const char* __restrict__ text, uint64_t n_quads, void* __restrict__ out,
                                                              uint64_t* __restrict__ report) {
    const uint64_t key = report[R_KEY];
    if (key != kNoKey) {                                             // refused: the report only
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            report[R_STATUS] = key & 0xFF;
            report[R_OFFSET] = key >> 8;
            report[R_VALUES] = 0;
        }
        return;
    }
    const uint64_t g = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (g * kGroupQuads >= n_quads) return;
    const uint64_t n_values = report[R_VALUES];
    uint32_t quads[kGroupQuads];
    load_quads(text, g, n_quads, quads);
    uint64_t w[3];
    decode_group(quads, w);
    if constexpr (DT == HMM_BASE64_DTYPE_F64) {
        uint64_t* o = static_cast<uint64_t*>(out);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (g * 3 + k < n_values) o[g * 3 + k] = w[k];
    } else if constexpr (DT == HMM_BASE64_DTYPE_F32) {
        float* o = static_cast<float*>(out);
        uint32_t inexact = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (g * 3 + k < n_values) {
                uint32_t bad;
                o[g * 3 + k] = narrow(w[k], &bad);
                inexact += bad;
            }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) inexact += __shfl_xor(inexact, off, 64);
        if ((threadIdx.x & 63) == 0 && inexact) atomicAdd(reinterpret_cast<unsigned long long*>(report + R_INEXACT), (unsigned long long)inexact);
    } else {
        uint8_t* o = static_cast<uint8_t*>(out);
#pragma unroll
        for (int i = 0; i < kGroupBytes; ++i)
            if (g * kGroupBytes + i < n_values) o[g * kGroupBytes + i] = (uint8_t)group_byte(w, i);
    }
}

bool known_dtype(int dtype) { return dtype == HMM_BASE64_DTYPE_F32 || dtype == HMM_BASE64_DTYPE_F64 || dtype == HMM_BASE64_DTYPE_U8; }
size_t source_align(int dtype) { return dtype == HMM_BASE64_DTYPE_F64 ? 8 : dtype == HMM_BASE64_DTYPE_F32 ? 4 : 1; }
size_t encoded_bytes_per_value(int dtype) { return dtype == HMM_BASE64_DTYPE_U8 ? 1 : 8; }
bool aligned(const void* p, size_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

// the checks both encoders share; `who` names the entry point
int check_encode_args(const char* who, const void* src, int dtype, size_t n_values, char* out, size_t cap, bool device) {
    HMM_REQUIRE(known_dtype(dtype), HMM_E_INVALID, "%s: dtype must be %d (fp32), %d (fp64) or %d (bytes), got %d", who, HMM_BASE64_DTYPE_F32,
                HMM_BASE64_DTYPE_F64, HMM_BASE64_DTYPE_U8, dtype);
    HMM_REQUIRE(n_values <= HMM_BASE64_MAX_BYTES / encoded_bytes_per_value(dtype), HMM_E_INVALID, "%s: %zu values, at most %llu bytes are encoded in one call",
                who, n_values, (unsigned long long)HMM_BASE64_MAX_BYTES);
    HMM_REQUIRE((src && out) || n_values == 0, HMM_E_INVALID, "%s: null pointer", who);
    const size_t need = hmm_base64_encoded_length(n_values * encoded_bytes_per_value(dtype));
    HMM_REQUIRE(cap >= need, HMM_E_INVALID, "%s: buffer of %zu bytes, need %zu", who, cap, need);
    HMM_REQUIRE(aligned(src, source_align(dtype)), HMM_E_INVALID, "%s: the source must be aligned to its element", who);
    HMM_REQUIRE(!device || aligned(out, 16), HMM_E_INVALID, "%s: out_dev must be 16-byte aligned", who);
    return HMM_OK;
}

// a float dtype writes floor(3 q / 8) values when the text is whole doubles; bytes: the padding (at most 2) is known on the device only
size_t least_cap(int dtype, size_t n_quads) {
    return dtype == HMM_BASE64_DTYPE_U8 ? (n_quads ? n_quads * 3 - 2 : 0) : n_quads * 3 / 8;
}

int check_decode_args(const char* who, const char* text, size_t n_chars, int dtype, void* out, size_t cap_values, uint64_t* report, bool device) {
    HMM_REQUIRE(known_dtype(dtype), HMM_E_INVALID, "%s: dtype_out must be %d (fp32), %d (fp64) or %d (bytes), got %d", who, HMM_BASE64_DTYPE_F32,
                HMM_BASE64_DTYPE_F64, HMM_BASE64_DTYPE_U8, dtype);
    HMM_REQUIRE(report, HMM_E_INVALID, "%s: null report", who);
    HMM_REQUIRE(n_chars <= HMM_BASE64_MAX_BYTES / 3 * 4, HMM_E_INVALID, "%s: %zu characters, at most %llu are decoded in one call", who, n_chars,
                (unsigned long long)(HMM_BASE64_MAX_BYTES / 3 * 4));
    HMM_REQUIRE(text || n_chars == 0, HMM_E_INVALID, "%s: null text", who);
    const size_t need = n_chars % 4 ? 0 : least_cap(dtype, n_chars / 4);
    HMM_REQUIRE(out || need == 0, HMM_E_INVALID, "%s: null output", who);
    HMM_REQUIRE(cap_values >= need, HMM_E_INVALID, "%s: room for %zu values, need %zu", who, cap_values, need);
    HMM_REQUIRE(aligned(out, dtype == HMM_BASE64_DTYPE_F64 ? 8 : dtype == HMM_BASE64_DTYPE_F32 ? 4 : 1) && aligned(report, 8), HMM_E_INVALID,
                "%s: the output must be aligned to its element and the report to 8 bytes", who);
    HMM_REQUIRE(!device || aligned(text, 16), HMM_E_INVALID, "%s: text_dev must be 16-byte aligned", who);
    return HMM_OK;
}

}  // namespace

extern "C" size_t hmm_base64_encoded_length(size_t n_bytes) { return (n_bytes + 2) / 3 * 4; }

extern "C" int hmm_base64_encode_device(const void* src_dev, int dtype, size_t n_values, char* out_dev, size_t cap, hmm_stream_t stream) {
    if (int rc = check_encode_args("base64_encode_device", src_dev, dtype, n_values, out_dev, cap, true)) return rc;
    if (n_values == 0) return HMM_OK;
    const uint64_t n_bytes = (uint64_t)n_values * encoded_bytes_per_value(dtype);
    const uint64_t groups = (n_bytes + kGroupBytes - 1) / kGroupBytes;
    const unsigned blocks = (unsigned)((groups + kThreads - 1) / kThreads);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dtype == HMM_BASE64_DTYPE_F64)
        b64_encode_kernel<HMM_BASE64_DTYPE_F64><<<blocks, kThreads, 0, st>>>(src_dev, n_values, n_bytes, out_dev);
    else if (dtype == HMM_BASE64_DTYPE_F32)
        b64_encode_kernel<HMM_BASE64_DTYPE_F32><<<blocks, kThreads, 0, st>>>(src_dev, n_values, n_bytes, out_dev);
    else
        b64_encode_kernel<HMM_BASE64_DTYPE_U8><<<blocks, kThreads, 0, st>>>(src_dev, n_values, n_bytes, out_dev);
    HMM_LAUNCH_CHECK();
    return HMM_OK;
}

extern "C" int hmm_base64_decode_device(const char* text_dev, size_t n_chars, int dtype_out, void* out_dev, size_t cap_values, uint64_t* report_dev,
                                        hmm_stream_t stream) {
    if (int rc = check_decode_args("base64_decode_device", text_dev, n_chars, dtype_out, out_dev, cap_values, report_dev, true)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n_chars % 4 || n_chars == 0) {                               // nothing to read: the report says which
        const bool bad = n_chars % 4 != 0;
        b64_report_init<<<1, 64, 0, st>>>(report_dev, bad ? HMM_BASE64_BAD_LENGTH : HMM_BASE64_OK, bad ? n_chars - n_chars % 4 : 0,
                                          bad ? key_of(n_chars - n_chars % 4, HMM_BASE64_BAD_LENGTH) : kNoKey);
        HMM_LAUNCH_CHECK();
        return HMM_OK;
    }
    const uint64_t n_quads = n_chars / 4;
    const uint64_t groups = (n_quads + kGroupQuads - 1) / kGroupQuads;
    const unsigned blocks = (unsigned)((groups + kThreads - 1) / kThreads);
    b64_report_init<<<1, 64, 0, st>>>(report_dev, HMM_BASE64_OK, 0, kNoKey);
    HMM_LAUNCH_CHECK();
    b64_check_kernel<<<blocks, kThreads, 0, st>>>(text_dev, n_quads, dtype_out, cap_values, report_dev);
    HMM_LAUNCH_CHECK();
    if (dtype_out == HMM_BASE64_DTYPE_F64)
        b64_decode_kernel<HMM_BASE64_DTYPE_F64><<<blocks, kThreads, 0, st>>>(text_dev, n_quads, out_dev, report_dev);
    else if (dtype_out == HMM_BASE64_DTYPE_F32)
        b64_decode_kernel<HMM_BASE64_DTYPE_F32><<<blocks, kThreads, 0, st>>>(text_dev, n_quads, out_dev, report_dev);
    else
        b64_decode_kernel<HMM_BASE64_DTYPE_U8><<<blocks, kThreads, 0, st>>>(text_dev, n_quads, out_dev, report_dev);
    HMM_LAUNCH_CHECK();
    return HMM_OK;
}

// ---- the same core on the host: no GPU call ---------------------------------------------------------------------------------
extern "C" int hmm_base64_encode_host(const void* src, int dtype, size_t n_values, char* out, size_t cap) {
    if (int rc = check_encode_args("base64_encode_host", src, dtype, n_values, out, cap, false)) return rc;
    const uint64_t n_bytes = (uint64_t)n_values * encoded_bytes_per_value(dtype);
    for (uint64_t g = 0; g * kGroupBytes < n_bytes; ++g) {
        const uint64_t left = n_bytes - g * kGroupBytes;
        const uint32_t here = left < (uint64_t)kGroupBytes ? (uint32_t)left : (uint32_t)kGroupBytes;
        uint64_t w[3] = {0, 0, 0};
        for (uint32_t i = 0; i < here; ++i) {
            uint32_t byte;
            const uint64_t at = g * kGroupBytes + i;
            if (dtype == HMM_BASE64_DTYPE_U8) byte = static_cast<const uint8_t*>(src)[at];
            else {
                const uint64_t bits = dtype == HMM_BASE64_DTYPE_F64 ? bits_of(static_cast<const double*>(src)[at / 8])
                                                                    : bits_of((double)static_cast<const float*>(src)[at / 8]);
                byte = (uint32_t)(bits >> (8 * (at % 8))) & 0xFF;
            }
            w[i >> 3] |= (uint64_t)byte << (8 * (i & 7));
        }
        uint32_t quads[kGroupQuads];
        encode_group(w, here, quads);
        for (uint32_t q = 0; q < (here + 2) / 3; ++q)
            for (int c = 0; c < 4; ++c) out[g * kGroupChars + q * 4 + c] = (char)((quads[q] >> (8 * c)) & 0xFF);
    }
    return HMM_OK;
}

extern "C" int hmm_base64_decode_host(const char* text, size_t n_chars, int dtype_out, void* out, size_t cap_values, uint64_t* report) {
    if (int rc = check_decode_args("base64_decode_host", text, n_chars, dtype_out, out, cap_values, report, false)) return rc;
    for (int i = 0; i < HMM_BASE64_REPORT_WORDS; ++i) report[i] = 0;
    report[R_KEY] = kNoKey;
    uint64_t key = kNoKey, n_values = 0;
    const uint64_t n_quads = n_chars / 4;
    auto quad_at = [&](uint64_t Q) {
        uint32_t quad = 0;
        for (int c = 0; c < 4; ++c) quad |= (uint32_t)(uint8_t)text[Q * 4 + c] << (8 * c);
        return quad;
    };
    if (n_chars % 4) key = key_of(n_chars - n_chars % 4, HMM_BASE64_BAD_LENGTH);
    for (uint64_t Q = 0; Q < n_quads && key == kNoKey; ++Q) {
        uint32_t pad;
        const bool last = Q + 1 == n_quads;
        key = check_quad(quad_at(Q), Q * 4, last, &pad);
        if (last && key == kNoKey) {
            const uint32_t status = count_values(n_quads, pad, dtype_out, cap_values, &n_values);
            if (status != HMM_BASE64_OK) key = key_of(Q * 4, status);
        }
    }
    report[R_KEY] = key;
    if (key != kNoKey) {
        report[R_STATUS] = key & 0xFF;
        report[R_OFFSET] = key >> 8;
        return HMM_OK;
    }
    report[R_VALUES] = n_values;
    for (uint64_t g = 0; g * kGroupQuads < n_quads; ++g) {
        uint32_t quads[kGroupQuads];
        for (int q = 0; q < kGroupQuads; ++q) quads[q] = g * kGroupQuads + q < n_quads ? quad_at(g * kGroupQuads + q) : 0x41414141u;
        uint64_t w[3];
        decode_group(quads, w);
        for (int k = 0; k < 3 && dtype_out != HMM_BASE64_DTYPE_U8; ++k) {
            if (g * 3 + k >= n_values) break;
            if (dtype_out == HMM_BASE64_DTYPE_F64) static_cast<uint64_t*>(out)[g * 3 + k] = w[k];
            else {
                uint32_t bad;
                static_cast<float*>(out)[g * 3 + k] = narrow(w[k], &bad);
                report[R_INEXACT] += bad;
            }
        }
        for (int i = 0; i < kGroupBytes && dtype_out == HMM_BASE64_DTYPE_U8; ++i)
            if (g * kGroupBytes + i < n_values) static_cast<uint8_t*>(out)[g * kGroupBytes + i] = (uint8_t)group_byte(w, i);
    }
    return HMM_OK;
}
