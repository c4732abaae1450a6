// Base64 (RFC 4648, standard alphabet, '=' padding) as the checkpoint file uses it (hippomm/core/hippocampal_memory.py:308-318,
// :1506): one core for the kernels of base64.hip and for the host twins behind hmm_base64_encode_host / hmm_base64_decode_host.
//
// The unit is a GROUP: 24 source bytes (three doubles) <-> 32 characters (eight quads of four).  A group is handed over as three
// 64-bit words in memory order (little endian: byte i of the group is bits 8 (i % 8) .. of word i / 8) and eight 32-bit words of
// four characters each, so that a full group leaves as two 16-byte stores.  Every loop below has constant bounds and unrolls:
// nothing is indexed by a run-time value, nothing goes to scratch.
#pragma once
#include <stdint.h>
#include "hippomm_hip.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HMM_B64_HD __host__ __device__ __forceinline__
#else
#define HMM_B64_HD inline
#endif

namespace hmm_b64 {

constexpr int kGroupBytes = HMM_BASE64_BYTES_PER_THREAD;        // 24
constexpr int kGroupChars = kGroupBytes / 3 * 4;                // 32
constexpr int kGroupQuads = kGroupChars / 4;                    // 8
constexpr uint64_t kNoKey = ~0ull;                              // no offending byte: above every (offset << 8 | status)

HMM_B64_HD uint64_t key_of(uint64_t offset, uint32_t status) { return (offset << 8) | status; }

// six bits -> their character
HMM_B64_HD uint32_t enc6(uint32_t v) {
    return v < 26 ? 'A' + v : v < 52 ? 'a' + (v - 26) : v < 62 ? '0' + (v - 52) : v == 62 ? '+' : '/';
}
// a character -> its six bits; 64 for '=', 65 for everything outside the alphabet
HMM_B64_HD uint32_t dec6(uint32_t c) {
    return (c >= 'A' && c <= 'Z') ? c - 'A' : (c >= 'a' && c <= 'z') ? c - 'a' + 26 : (c >= '0' && c <= '9') ? c - '0' + 52
           : c == '+' ? 62 : c == '/' ? 63 : c == '=' ? 64 : 65;
}

HMM_B64_HD uint32_t group_byte(const uint64_t w[3], int i) { return (uint32_t)(w[i >> 3] >> (8 * (i & 7))) & 0xFFu; }

// Bytes [0, n_bytes) of a group (1 <= n_bytes <= 24; the bytes behind n_bytes are zero in w) -> quads[0, (n_bytes + 2) / 3), the
// last of them padded with '=' when n_bytes is no multiple of three.  The quads behind that are not meaningful.
HMM_B64_HD void encode_group(const uint64_t w[3], uint32_t n_bytes, uint32_t quads[kGroupQuads]) {
#pragma unroll
    for (int q = 0; q < kGroupQuads; ++q) {
        const uint32_t b0 = group_byte(w, 3 * q), b1 = group_byte(w, 3 * q + 1), b2 = group_byte(w, 3 * q + 2);
        uint32_t c0 = enc6(b0 >> 2), c1 = enc6(((b0 & 3) << 4) | (b1 >> 4)), c2 = enc6(((b1 & 15) << 2) | (b2 >> 6)), c3 = enc6(b2 & 63);
        if (n_bytes == (uint32_t)(3 * q + 1)) c2 = '=';
        if (n_bytes == (uint32_t)(3 * q + 1) || n_bytes == (uint32_t)(3 * q + 2)) c3 = '=';
        quads[q] = c0 | (c1 << 8) | (c2 << 16) | (c3 << 24);
    }
}

// The strict rules, position by position.  quad: the four characters at text offset `at`; last: it is the text's last quad (the
// only place padding may stand).  Returns the key (offset << 8 | status) of the first position that breaks a rule, kNoKey if none
// does; *pad receives the quad's padding characters (0 in a quad that is not the last).
HMM_B64_HD uint64_t check_quad(uint32_t quad, uint64_t at, bool last, uint32_t* pad) {
    const uint32_t v0 = dec6(quad & 0xFF), v1 = dec6((quad >> 8) & 0xFF), v2 = dec6((quad >> 16) & 0xFF), v3 = dec6(quad >> 24);
    *pad = 0;
    if (v0 >= 64) return key_of(at, v0 == 64 ? HMM_BASE64_BAD_PADDING : HMM_BASE64_BAD_CHAR);
    if (v1 >= 64) return key_of(at + 1, v1 == 64 ? HMM_BASE64_BAD_PADDING : HMM_BASE64_BAD_CHAR);
    if (!last) {
        if (v2 >= 64) return key_of(at + 2, v2 == 64 ? HMM_BASE64_BAD_PADDING : HMM_BASE64_BAD_CHAR);
        if (v3 >= 64) return key_of(at + 3, v3 == 64 ? HMM_BASE64_BAD_PADDING : HMM_BASE64_BAD_CHAR);
        return kNoKey;
    }
    if (v2 == 64 && v3 == 64 && (v1 & 15)) return key_of(at + 1, HMM_BASE64_NONCANONICAL);     // "xx==": four unused bits
    if (v2 == 65) return key_of(at + 2, HMM_BASE64_BAD_CHAR);
    if (v2 == 64 && v3 != 64) return key_of(at + 2, HMM_BASE64_BAD_PADDING);                    // "xx=x"
    if (v2 < 64 && v3 == 64 && (v2 & 3)) return key_of(at + 2, HMM_BASE64_NONCANONICAL);        // "xxx=": two unused bits
    if (v3 == 65) return key_of(at + 3, HMM_BASE64_BAD_CHAR);
    *pad = (v2 == 64 ? 1u : 0u) + (v3 == 64 ? 1u : 0u);
    return kNoKey;
}

// Eight checked quads (padding decodes as zero bits) -> the 24 bytes of their group.
HMM_B64_HD void decode_group(const uint32_t quads[kGroupQuads], uint64_t w[3]) {
    w[0] = w[1] = w[2] = 0;
#pragma unroll
    for (int q = 0; q < kGroupQuads; ++q) {
        const uint32_t v0 = dec6(quads[q] & 0xFF) & 63, v1 = dec6((quads[q] >> 8) & 0xFF) & 63, v2 = dec6((quads[q] >> 16) & 0xFF) & 63,
                       v3 = dec6(quads[q] >> 24) & 63;
        const uint32_t b[3] = {(v0 << 2) | (v1 >> 4), ((v1 & 15) << 4) | (v2 >> 2), ((v2 & 3) << 6) | v3};
#pragma unroll
        for (int k = 0; k < 3; ++k) w[(3 * q + k) >> 3] |= (uint64_t)b[k] << (8 * ((3 * q + k) & 7));
    }
}

// What the last quad says about the whole text: n_quads quads, `pad` padding characters, as `dtype` -> the number of values in
// *n_values, or the status that refuses the text (a float dtype needs whole doubles; the caller's buffer must hold them).
HMM_B64_HD uint32_t count_values(uint64_t n_quads, uint32_t pad, int dtype, uint64_t cap_values, uint64_t* n_values) {
    const uint64_t n_bytes = n_quads * 3 - pad;
    *n_values = dtype == HMM_BASE64_DTYPE_U8 ? n_bytes : n_bytes / 8;
    if (dtype != HMM_BASE64_DTYPE_U8 && n_bytes % 8) return HMM_BASE64_PARTIAL_VALUE;
    if (*n_values > cap_values) return HMM_BASE64_CAPACITY;
    return HMM_BASE64_OK;
}

HMM_B64_HD uint64_t bits_of(double d) {
    union { double d; uint64_t u; } x;
    x.d = d;
    return x.u;
}
HMM_B64_HD double double_of(uint64_t u) {
    union { double d; uint64_t u; } x;
    x.u = u;
    return x.d;
}
// a decoded double narrowed to fp32; *inexact: widening the result does not give the same 64 bits back
HMM_B64_HD float narrow(uint64_t bits, uint32_t* inexact) {
    const float f = (float)double_of(bits);
    *inexact = bits_of((double)f) != bits ? 1u : 0u;
    return f;
}

}  // namespace hmm_b64
