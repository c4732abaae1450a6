// float.__repr__ of a double, for the host and for the gfx950 kernels of event_json.hip: the characters json.dumps writes for a
// float (hippomm/core/hippocampal_memory.py:331-335 writes every stored feature through it).
//
// Finite values: the shortest decimal digit string that reads back as the same double, the closest to the value among the
// shortest (Python's dtoa mode 0), in fixed notation when -4 < decpt <= 16 and as d[.ddd]e+XX otherwise (decpt: the position of the
// decimal point, value = 0.d1d2... x 10^decpt) -- the rule py_float_repr in event_json.cpp states, which stays the second oracle.
// 0.0, -0.0, NaN, Infinity and -Infinity as json.dumps spells them.  At most HMM_JSON_REPR_MAX = 24 characters
// ("-1.2345678901234567e-308").
//
// The digits come from the Ryu construction (Adams, PLDI 2018): with the double as m2 * 2^e2, the value and the two halfway
// points to its neighbours (4 m2, 4 m2 + 2, 4 m2 - 1 or - 2) are scaled by 10^-q with one 64 x 128-bit multiply each, q chosen so
// that the three integers keep every digit that can matter; digits are then removed while the interval still holds a shorter
// number, with the exact "all removed digits were zero" facts that decide ties.  The factors are the project's own tables
// (event_json_tables.h, written by tools/gen_event_json_tables.py); the caller says where they lie, so that the device reads them
// from global memory and the host from its own copy.  Correct for every double, not only widened fp32 (a reloaded event holds
// float64): tests/test_cpu_event_json_device.py walks every binary exponent and millions of bit patterns against repr().
//
// Split in two so that a kernel can place text before it forms it: hmm_json_decompose (the arithmetic, all in registers),
// hmm_json_repr_length and hmm_json_repr_emit (bytes through a pointer, LDS on the device).
#pragma once
#include <stdint.h>
#include "event_json_tables.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HMM_JSON_HD __host__ __device__ inline
#else
#define HMM_JSON_HD inline
#endif

#define HMM_JSON_REPR_MAX 24

namespace hmm_json {

enum Kind : int { kFinite = 0, kZero = 1, kInf = 2, kNaN = 3 };

struct Decimal {
    uint64_t digits;   // kFinite: the significant digits as an integer, 1 .. 17 of them, no trailing zero unless it is the only digit
    int ndigits;
    int decpt;         // value = 0.d1d2...dn x 10^decpt
    int kind;
    int negative;      // the sign bit (never set for NaN: json writes "NaN")
};

HMM_JSON_HD uint64_t umulh(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// (m * (mul[1] << 64 | mul[0])) >> j for 64 < j < 128: the product's bits below 2^64 of the low partial product cannot reach the result.
HMM_JSON_HD uint64_t mul_shift(uint64_t m, const uint64_t* mul, int j) {
    const uint64_t b0_hi = umulh(m, mul[0]);
    const uint64_t b2_lo = m * mul[1], b2_hi = umulh(m, mul[1]);
    const uint64_t lo = b0_hi + b2_lo;
    const uint64_t hi = b2_hi + (lo < b0_hi ? 1u : 0u);
    const int s = j - 64;
    return s == 0 ? lo : (lo >> s) | (hi << (64 - s));
}

HMM_JSON_HD int pow5_bits(int e) { return (int)(((uint32_t)e * 1217359u) >> 19) + 1; }     // bit length of 5^e, 0 <= e <= 3528
HMM_JSON_HD int log10_pow2(int e) { return (int)(((uint32_t)e * 78913u) >> 18); }          // floor(e log10 2), 0 <= e <= 1650
HMM_JSON_HD int log10_pow5(int e) { return (int)(((uint32_t)e * 732923u) >> 20); }         // floor(e log10 5), 0 <= e <= 2620

HMM_JSON_HD bool multiple_of_pow5(uint64_t v, int p) {
    int n = 0;
    for (;;) {
        const uint64_t q = v / 5;
        if (v - 5 * q != 0) break;
        v = q;
        ++n;
    }
    return n >= p;
}

HMM_JSON_HD int decimal_length17(uint64_t v) {
    if (v >= 10000000000000000ull) return 17;
    if (v >= 1000000000000000ull) return 16;
    if (v >= 100000000000000ull) return 15;
    if (v >= 10000000000000ull) return 14;
    if (v >= 1000000000000ull) return 13;
    if (v >= 100000000000ull) return 12;
    if (v >= 10000000000ull) return 11;
    if (v >= 1000000000ull) return 10;
    if (v >= 100000000ull) return 9;
    if (v >= 10000000ull) return 8;
    if (v >= 1000000ull) return 7;
    if (v >= 100000ull) return 6;
    if (v >= 10000ull) return 5;
    if (v >= 1000ull) return 4;
    if (v >= 100ull) return 3;
    if (v >= 10ull) return 2;
    return 1;
}

// pow5_inv: HMM_JSON_POW5_INV_COUNT x 2 words, pow5: HMM_JSON_POW5_COUNT x 2 words (event_json_tables.h).
HMM_JSON_HD Decimal decompose(double x, const uint64_t (*pow5_inv)[2], const uint64_t (*pow5)[2]) {
    uint64_t bits;
    __builtin_memcpy(&bits, &x, 8);
    const uint64_t mantissa = bits & ((1ull << 52) - 1);
    const int exponent = (int)((bits >> 52) & 0x7FF);
    Decimal d;
    d.digits = 0;
    d.ndigits = 1;
    d.decpt = 1;
    d.negative = (int)(bits >> 63);
    if (exponent == 0x7FF) {
        d.kind = mantissa ? kNaN : kInf;
        if (mantissa) d.negative = 0;
        return d;
    }
    if (exponent == 0 && mantissa == 0) {
        d.kind = kZero;
        return d;
    }
    d.kind = kFinite;
    // the value is m2 * 2^e2; two more binary places make room for the halfway points
    const int e2 = (exponent ? exponent : 1) - 1023 - 52 - 2;
    const uint64_t m2 = exponent ? (1ull << 52) | mantissa : mantissa;
    const bool accept_bounds = (m2 & 1) == 0;                  // round-half-even reads a halfway point back as the even neighbour
    const uint64_t mv = 4 * m2;
    const uint32_t mm_shift = (mantissa != 0 || exponent <= 1) ? 1u : 0u;     // the lower neighbour is half as far at a power of two
    uint64_t vr, vp, vm;
    int e10;
    bool vm_trailing_zeros = false, vr_trailing_zeros = false;
    if (e2 >= 0) {
        const int q = log10_pow2(e2) - (e2 > 3 ? 1 : 0);
        e10 = q;
        const int k = HMM_JSON_POW5_BITS + pow5_bits(q) - 1;
        const int j = -e2 + q + k;
        const uint64_t* mul = pow5_inv[q];
        vr = mul_shift(4 * m2, mul, j);
        vp = mul_shift(4 * m2 + 2, mul, j);
        vm = mul_shift(4 * m2 - 1 - mm_shift, mul, j);
        if (q <= 21) {                                         // only then can mv, mp or mm be a multiple of 5^q (they are below 2^55)
            const uint32_t mv_mod5 = (uint32_t)(mv - 5 * (mv / 5));
            if (mv_mod5 == 0) vr_trailing_zeros = multiple_of_pow5(mv, q);
            else if (accept_bounds) vm_trailing_zeros = multiple_of_pow5(mv - 1 - mm_shift, q);
            else vp -= multiple_of_pow5(mv + 2, q) ? 1u : 0u;
        }
    } else {
        const int q = log10_pow5(-e2) - (-e2 > 1 ? 1 : 0);
        e10 = q + e2;
        const int i = -e2 - q;
        const int k = pow5_bits(i) - HMM_JSON_POW5_BITS;
        const int j = q - k;
        const uint64_t* mul = pow5[i];
        vr = mul_shift(4 * m2, mul, j);
        vp = mul_shift(4 * m2 + 2, mul, j);
        vm = mul_shift(4 * m2 - 1 - mm_shift, mul, j);
        if (q <= 1) {
            vr_trailing_zeros = true;                          // mv = 4 m2 has at least two factors of two
            if (accept_bounds) vm_trailing_zeros = mm_shift == 1;
            else --vp;
        } else if (q < 63) {
            vr_trailing_zeros = (mv & ((1ull << q) - 1)) == 0;
        }
    }
    int removed = 0;
    uint32_t last_removed = 0;
    uint64_t out;
    if (vm_trailing_zeros || vr_trailing_zeros) {              // rare: exact ties and exact ends of the interval
        for (;;) {
            const uint64_t vp10 = vp / 10, vm10 = vm / 10;
            if (vp10 <= vm10) break;
            const uint64_t vr10 = vr / 10;
            vm_trailing_zeros &= (vm - 10 * vm10) == 0;
            vr_trailing_zeros &= last_removed == 0;
            last_removed = (uint32_t)(vr - 10 * vr10);
            vr = vr10; vp = vp10; vm = vm10;
            ++removed;
        }
        if (vm_trailing_zeros) {
            for (;;) {
                const uint64_t vm10 = vm / 10;
                if (vm - 10 * vm10 != 0) break;
                const uint64_t vp10 = vp / 10, vr10 = vr / 10;
                vr_trailing_zeros &= last_removed == 0;
                last_removed = (uint32_t)(vr - 10 * vr10);
                vr = vr10; vp = vp10; vm = vm10;
                ++removed;
            }
        }
        if (vr_trailing_zeros && last_removed == 5 && (vr & 1) == 0) last_removed = 4;      // exactly halfway: to even
        out = vr + (((vr == vm && (!accept_bounds || !vm_trailing_zeros)) || last_removed >= 5) ? 1u : 0u);
    } else {
        bool round_up = false;
        for (;;) {
            const uint64_t vp10 = vp / 10, vm10 = vm / 10;
            if (vp10 <= vm10) break;
            const uint64_t vr10 = vr / 10;
            round_up = (uint32_t)(vr - 10 * vr10) >= 5;
            vr = vr10; vp = vp10; vm = vm10;
            ++removed;
        }
        out = vr + ((vr == vm || round_up) ? 1u : 0u);
    }
    d.digits = out;
    d.ndigits = decimal_length17(out);
    d.decpt = e10 + removed + d.ndigits;
    return d;
}

HMM_JSON_HD int repr_length(const Decimal& d) {
    if (d.kind == kNaN) return 3;
    if (d.kind == kInf) return 8 + d.negative;
    if (d.kind == kZero) return 3 + d.negative;
    const int n = d.ndigits, decpt = d.decpt;
    int len;
    if (decpt <= -4 || decpt > 16) {
        const int e = decpt - 1 < 0 ? 1 - decpt : decpt - 1;
        len = n + (n > 1 ? 1 : 0) + 2 + (e >= 100 ? 3 : 2);
    } else if (decpt <= 0) {
        len = 2 - decpt + n;
    } else if (decpt >= n) {
        len = decpt + 2;
    } else {
        len = n + 1;
    }
    return len + d.negative;
}

// Writes repr_length(d) characters at out and returns that count.  P: a pointer to char in whatever address space.
template <typename P>
HMM_JSON_HD int repr_emit(const Decimal& d, P out) {
    int at = 0;
    if (d.kind == kNaN) { out[0] = 'N'; out[1] = 'a'; out[2] = 'N'; return 3; }
    if (d.negative) out[at++] = '-';
    if (d.kind == kInf) {
        const char* s = "Infinity";
        for (int i = 0; i < 8; ++i) out[at + i] = s[i];
        return at + 8;
    }
    if (d.kind == kZero) { out[at] = '0'; out[at + 1] = '.'; out[at + 2] = '0'; return at + 3; }
    const int n = d.ndigits, decpt = d.decpt;
    uint64_t v = d.digits;
    if (decpt <= -4 || decpt > 16) {
        // d[.ddd]e+XX: the digits from the right, the point after the first
        const int tail = n > 1 ? n : 0;                       // characters after the first digit, the point included
        for (int i = n - 1; i >= 1; --i) {
            const uint64_t q = v / 10;
            out[at + 1 + i] = (char)('0' + (int)(v - 10 * q));
            v = q;
        }
        out[at] = (char)('0' + (int)v);
        if (n > 1) out[at + 1] = '.';
        at += 1 + tail;
        out[at++] = 'e';
        int e = decpt - 1;
        out[at++] = e < 0 ? '-' : '+';
        if (e < 0) e = -e;
        if (e >= 100) { out[at++] = (char)('0' + e / 100); e %= 100; }
        out[at++] = (char)('0' + e / 10);
        out[at++] = (char)('0' + e % 10);
        return at;
    }
    if (decpt <= 0) {                                         // 0.000ddd
        out[at++] = '0';
        out[at++] = '.';
        for (int i = 0; i < -decpt; ++i) out[at++] = '0';
        for (int i = n - 1; i >= 0; --i) {
            const uint64_t q = v / 10;
            out[at + i] = (char)('0' + (int)(v - 10 * q));
            v = q;
        }
        return at + n;
    }
    if (decpt >= n) {                                         // ddd000.0
        for (int i = n - 1; i >= 0; --i) {
            const uint64_t q = v / 10;
            out[at + i] = (char)('0' + (int)(v - 10 * q));
            v = q;
        }
        at += n;
        for (int i = n; i < decpt; ++i) out[at++] = '0';
        out[at++] = '.';
        out[at++] = '0';
        return at;
    }
    for (int i = n; i >= 0; --i) {                            // dd.ddd: position decpt holds the point
        if (i == decpt) { out[at + i] = '.'; continue; }
        const uint64_t q = v / 10;
        out[at + i] = (char)('0' + (int)(v - 10 * q));
        v = q;
    }
    return at + n + 1;
}

// A double in, the characters json.dumps writes for it out (at most HMM_JSON_REPR_MAX), and their count.
template <typename P>
HMM_JSON_HD int float_repr(double x, P out, const uint64_t (*pow5_inv)[2], const uint64_t (*pow5)[2]) {
    return repr_emit(decompose(x, pow5_inv, pow5), out);
}

}  // namespace hmm_json
