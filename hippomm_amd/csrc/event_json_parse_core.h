// float(token) of one JSON number token, for the host and for the gfx950 kernels of event_json_parse.hip: the IEEE double Python's
// float() gives for the characters (correctly rounded), as 64 bits, and from it the fp32 (float)(double) -- the contract of
// hmm_json_parse_matrix_f32 (event_json.cpp: convert_number) and what np.array(json.load(f)).astype(np.float32) holds.
//
// Grammar: JSON's numbers as scan_number in event_json.cpp states them (-? (0 | [1-9][0-9]*) (. [0-9]+)? ([eE] [+-]? [0-9]+)?), and
// the three literals Python's json writes: NaN (0x7ff8000000000000 / 0x7fc00000), Infinity, -Infinity.  No leading '+', no ".5", no
// "1.", no hex.  "-0.0" and "-0e0" keep the sign; "-0" and every other zero without '.' or exponent is an int to json.load: +0.0.
//
// Conversion: Eisel-Lemire.  The first 19 significant digits (counted from the first non-zero digit of the mantissa) are an integer
// w < 10^19 < 2^64, the literal is w x 10^q.  w is normalised to 64 bits and multiplied by the 128-bit significand of 5^q
// (event_json_parse_tables.h); the top 54 bits of the product, the binary exponent from floor(q log2 10) and one round-to-nearest-
// even step are the double.  With the table's roundings the truncated product decides the rounding for EVERY w < 2^64 and q -- no
// fallback exists or is needed (Mushtak & Lemire, "Fast number parsing without fallback", SPE 2023) -- so a literal of at most 19
// significant digits inside the double range is always converted, exactly.  Integer arithmetic throughout: no fp64 operation whose
// result could depend on contraction or the float mode.
//
// What is NOT converted comes back as a flag, never as a value:
//   kUndecided   more than 19 significant digits, and w and w + 1 (the literal lies between them) round to different doubles;
//   kOutOfRange  a non-zero literal that rounds to infinity or to zero, or a decimal exponent above 9999 (more than four digits);
//                the host parser declines the file there (from_chars: result_out_of_range) and json.load answers;
//   kTooLong     a token of more than HMM_JSON_TOKEN_MAX bytes (decided by the caller, which knows the length before it reads);
//   kBadToken    not a number by the grammar above.
#pragma once
#include <stdint.h>
#include "event_json_core.h"
#include "event_json_parse_tables.h"

#ifndef HMM_JSON_TOKEN_MAX
#define HMM_JSON_TOKEN_MAX 64                                  // include/hippomm_hip.h states the same
#endif

namespace hmm_json {

enum ParseFlag : int { kParsed = 0, kUndecided = 1, kOutOfRange = 2, kTooLong = 3, kBadToken = 4 };

constexpr uint64_t kInfBits = 0x7FF0000000000000ull;
constexpr uint64_t kNaNBits = 0x7FF8000000000000ull;

HMM_JSON_HD int leading_zeros64(uint64_t x) {                  // x != 0
#if defined(__HIP_DEVICE_COMPILE__)
    return __clzll((long long)x);
#else
    return __builtin_clzll(x);
#endif
}

// The double nearest to w x 10^q (ties to even) as bits without a sign, w != 0: 0 when it rounds to zero, kInfBits when it overflows.
// pow10: HMM_JSON_POW10_COUNT x 2 words (event_json_parse_tables.h).
HMM_JSON_HD uint64_t decimal_to_double_bits(uint64_t w, int q, const uint64_t (*pow10)[2]) {
    if (q < HMM_JSON_POW10_MIN_Q) return 0;
    if (q > HMM_JSON_POW10_MAX_Q) return kInfBits;
    const int lz = leading_zeros64(w);
    w <<= lz;
    const uint64_t* f = pow10[q - HMM_JSON_POW10_MIN_Q];
    // the top 128 bits of w x (f[1] : f[0]); the low partial product is needed only when the 9 bits below the kept 55 are all ones
    uint64_t lo = w * f[1], hi = umulh(w, f[1]);
    if ((hi & 0x1FF) == 0x1FF) {
        const uint64_t second = umulh(w, f[0]);
        lo += second;
        if (second > lo) ++hi;
    }
    const int upper = (int)(hi >> 63);
    const int shift = upper + 9;                               // 64 - 52 - 3: the significand, one guard bit
    uint64_t m = hi >> shift;
    // floor(q log2 10) + 63 from 217706 / 65536 (exact for |q| <= 342); q may be negative: floor division, not a shift of a negative int
    const int scaled = 217706 * q;
    const int log2_10q = scaled >= 0 ? scaled >> 16 : -((-scaled + 65535) >> 16);
    int e = log2_10q + 63 + upper - lz + 1023;
    if (e <= 0) {                                              // subnormal: the significand loses 1 - e bits before the rounding
        if (1 - e >= 64) return 0;
        m >>= 1 - e;
        m += m & 1;
        m >>= 1;
        return m;                                              // m == 2^52 (rounded up to the smallest normal) is its own encoding
    }
    // exactly halfway between two doubles: only when 5^q fits the product exactly, -4 <= q <= 23; then to even
    if (lo <= 1 && q >= -4 && q <= 23 && (m & 3) == 1 && (m << shift) == hi) m &= ~1ull;
    m += m & 1;
    m >>= 1;
    if (m >= (2ull << 52)) {
        m = 1ull << 52;
        ++e;
    }
    m &= ~(1ull << 52);
    if (e >= 0x7FF) return kInfBits;
    return ((uint64_t)e << 52) | m;
}

// (float)(double) on the bits, round to nearest even: what the cast instruction gives, NaN as 0x7fc00000.
HMM_JSON_HD uint32_t narrow_double_bits(uint64_t b) {
    const uint32_t sign = (uint32_t)(b >> 63) << 31;
    const int e = (int)((b >> 52) & 0x7FF);
    const uint64_t frac = b & ((1ull << 52) - 1);
    if (e == 0x7FF) return frac ? 0x7FC00000u : sign | 0x7F800000u;
    if (e == 0) return sign;                                   // a double subnormal is far below half the smallest fp32 subnormal
    const int ef = e - 1023 + 127;
    if (ef >= 255) return sign | 0x7F800000u;
    const uint64_t full = frac | (1ull << 52);
    const int shift = ef >= 1 ? 29 : 29 + 1 - ef;              // an fp32 subnormal keeps fewer bits
    if (shift >= 64) return sign;
    uint64_t keep = full >> shift;
    const uint64_t rest = full & ((1ull << shift) - 1), half = 1ull << (shift - 1);
    if (rest > half || (rest == half && (keep & 1))) ++keep;
    // normal: keep carries the implicit bit, which adds one to the exponent field below it; a carry out of the significand moves on
    // into the exponent, up to infinity -- and from the largest subnormal into the smallest normal
    const uint32_t field = ef >= 1 ? (uint32_t)(ef - 1) << 23 : 0u;
    return sign | (field + (uint32_t)keep);
}

HMM_JSON_HD bool is_digit(int c) { return c >= '0' && c <= '9'; }

// The token p[0 .. n) (1 <= n <= HMM_JSON_TOKEN_MAX; P: a pointer to char in whatever address space) -> *bits and kParsed, or
// a flag and *bits = 0.
template <typename P>
HMM_JSON_HD int parse_number(P p, int n, const uint64_t (*pow10)[2], uint64_t* bits) {
    *bits = 0;
    int i = 0;
    const bool neg = p[0] == '-';
    if (neg) ++i;
    if (n - i == 8) {
        const char* s = "Infinity";
        bool same = true;
        for (int j = 0; j < 8; ++j) same &= p[i + j] == s[j];
        if (same) { *bits = kInfBits | ((uint64_t)neg << 63); return kParsed; }
    }
    if (!neg && n == 3 && p[0] == 'N' && p[1] == 'a' && p[2] == 'N') { *bits = kNaNBits; return kParsed; }
    if (i >= n || !is_digit(p[i])) return kBadToken;
    uint64_t w = 0;
    int nd = 0, q = 0;                                         // significant digits seen; the literal is w x 10^q (plus what w dropped)
    if (p[i] == '0') {
        ++i;
    } else {
        for (; i < n && is_digit(p[i]); ++i) {
            if (nd < 19) w = w * 10 + (uint64_t)(p[i] - '0');
            else ++q;                                          // a dropped integer digit
            ++nd;
        }
    }
    bool real = false;                                         // a '.' or an exponent: a float to json.load
    if (i < n && p[i] == '.') {
        real = true;
        ++i;
        if (i >= n || !is_digit(p[i])) return kBadToken;
        for (; i < n && is_digit(p[i]); ++i) {
            const int d = p[i] - '0';
            if (nd == 0 && d == 0) { --q; continue; }          // zeros in front of the first significant digit
            if (nd < 19) { w = w * 10 + (uint64_t)d; --q; }
            ++nd;
        }
    }
    int e = 0;
    bool eneg = false;
    if (i < n && (p[i] == 'e' || p[i] == 'E')) {
        real = true;
        ++i;
        if (i < n && (p[i] == '+' || p[i] == '-')) { eneg = p[i] == '-'; ++i; }
        if (i >= n || !is_digit(p[i])) return kBadToken;
        for (; i < n && is_digit(p[i]); ++i)
            if (e < 100000) e = e * 10 + (p[i] - '0');
    }
    if (i != n) return kBadToken;
    if (e > 9999) return kOutOfRange;
    if (w == 0) { *bits = (neg && real) ? 1ull << 63 : 0; return kParsed; }
    q += eneg ? -e : e;
    const uint64_t r = decimal_to_double_bits(w, q, pow10);
    // more digits than w holds: the literal lies in [w, w + 1] x 10^q, and rounding is monotone
    if (nd > 19 && decimal_to_double_bits(w + 1, q, pow10) != r) return kUndecided;
    if (r == 0 || r == kInfBits) return kOutOfRange;
    *bits = r | ((uint64_t)neg << 63);
    return kParsed;
}

}  // namespace hmm_json
