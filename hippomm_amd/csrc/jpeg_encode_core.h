// What one thread of the baseline JPEG encoder does at each stage, as functions that compile for the host too: jpeg_encode.hip runs
// them on gfx950, tools/jpeg_encode_model.cpp runs them thread by thread under a sanitizer.  Everything restates libjpeg as
// libjpeg-turbo runs it under Pillow's defaults, so a file is Image.save(.., "JPEG", quality=q, subsampling=s)'s byte for byte:
//
//   pixels   jccolor.c's fixed-point RGB -> YCbCr (SCALEBITS 16); the right edge replicated at full resolution (jcsample.c's
//            expand_right_edge); the last row replicated at full resolution up to a whole row group of vs rows and, below that,
//            each component's last DOWNSAMPLED row (jcprepct.c); jcsample.c's h2v1 / h2v2 box filter with its alternating bias;
//            level shift; jfdctint.c (CONST_BITS 13, PASS1_BITS 2, output scaled by 8); jcdctmgr.c's quantisation
//            (|x| + divisor / 2) / divisor with the sign restored, divisor = 8 * table entry.
//   scan     jccoefct.c's MCU order with its dummy blocks: where the luma block grid ends inside the last MCU column or row, the
//            MCU is filled with blocks without AC whose DC is that of the block before them in the MCU.
//   entropy  jchuff.c's encode_one_block with the standard tables; the last byte padded with ones; FF followed by 00.
//
// Integer arithmetic only.  32-bit products suffice: a first-pass value is below 2^13, a constant below 2^15 and at most four
// products are summed.
#pragma once
#include <stdint.h>

#include "jpeg_layout.h"

#define HMM_HD __host__ __device__ __forceinline__

namespace hmm {

constexpr int kEncFdctBlocks = 32;             // blocks per workgroup of jpeg_fdct_kernel, 8 threads each
constexpr int kEncScanTile = 1024;             // threads of the one-workgroup-per-frame kernels: blocks per prefix-sum step
constexpr int kEncStuffBytes = 16;             // bitstream bytes per thread and step of the stuffing pass
constexpr int kEncEmitThreads = 256;

// ---- where a scan block lies ----------------------------------------------------------------------------------------------------
struct EncBlock {
    int32_t comp;                              // 0 Y, 1 Cb, 2 Cr
    int32_t bx, by;                            // the block of the component whose samples are transformed
    int32_t dummy;                             // 1: keep its DC only (bx, by is the block jccoefct.c copies the DC from)
};

HMM_HD EncBlock enc_block_at(const JpegEncLayout& L, uint32_t b) {
    EncBlock e{};
    if (L.ncomp == 1) {
        e.bx = (int32_t)(b % (uint32_t)L.mcux);
        e.by = (int32_t)(b / (uint32_t)L.mcux);
        return e;
    }
    const uint32_t mcu = b / (uint32_t)L.bpm;
    const int32_t k = (int32_t)(b - mcu * (uint32_t)L.bpm);
    const int32_t mx = (int32_t)(mcu % (uint32_t)L.mcux), my = (int32_t)(mcu / (uint32_t)L.mcux);
    const int32_t luma = L.hs * L.vs;
    if (k >= luma) {
        e.comp = 1 + k - luma;
        e.bx = mx;
        e.by = my;
        return e;
    }
    int32_t xi = k % L.hs, yi = k / L.hs;
    if (my * L.vs + yi >= L.hib) {             // a row of dummies: all copy the last block of the row above, itself maybe a dummy
        e.dummy = 1;
        yi -= 1;
        xi = L.hs - 1;
    }
    if (mx * L.hs + xi >= L.wib) {             // a dummy at the right edge copies the block on its left
        e.dummy = 1;
        xi -= 1;
    }
    e.bx = mx * L.hs + xi;
    e.by = my * L.vs + yi;
    return e;
}

// The block before block b in its component's scan order (the DC predictor), -1 for the component's first block.
HMM_HD int64_t enc_pred_block(const JpegEncLayout& L, uint32_t b) {
    if (L.ncomp == 1) return (int64_t)b - 1;
    const uint32_t k = b % (uint32_t)L.bpm;
    const uint32_t luma = (uint32_t)(L.hs * L.vs);
    if (k > 0 && k < luma) return (int64_t)b - 1;
    if (b < (uint32_t)L.bpm) return -1;
    return k == 0 ? (int64_t)b - 3 : (int64_t)b - L.bpm;              // luma: the last luma block of the MCU before
}

// ---- pixels -> samples ---------------------------------------------------------------------------------------------------------
// Pixel (x, y) of the frame, x and y inside it.  channels 1: grey; 3: RGB, or BGR when bgr.
HMM_HD int32_t enc_component(const uint8_t* __restrict__ frame, const JpegEncLayout& L, int channels, int bgr, int comp, int x, int y) {
    const uint8_t* p = frame + ((int64_t)y * L.w + x) * channels;
    if (channels == 1) return p[0];
    const int32_t r = bgr ? p[2] : p[0], g = p[1], b = bgr ? p[0] : p[2];
    if (comp == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    if (comp == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// Row t of block (bx, by) of component comp: 8 level-shifted samples.
HMM_HD void enc_sample_row(const uint8_t* __restrict__ frame, const JpegEncLayout& L, int channels, int bgr, int comp, int bx, int by,
                           int t, int32_t* d) {
    const int sy = by * 8 + t;
    if (comp == 0 || (L.hs == 1 && L.vs == 1)) {
        const int y = sy < L.h ? sy : L.h - 1;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int sx = bx * 8 + j;
            d[j] = enc_component(frame, L, channels, bgr, comp, sx < L.w ? sx : L.w - 1, y) - 128;
        }
        return;
    }
    const int cy = sy < L.ch ? sy : L.ch - 1;                          // below the image: the last downsampled row again
    const int y0 = cy * L.vs, y1 = y0 + 1 < L.h ? y0 + 1 : L.h - 1;    // inside it: the last row replicated at full resolution
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int sx = bx * 8 + j;
        const int x0 = 2 * sx < L.w ? 2 * sx : L.w - 1, x1 = 2 * sx + 1 < L.w ? 2 * sx + 1 : L.w - 1;
        int32_t v = enc_component(frame, L, channels, bgr, comp, x0, y0) + enc_component(frame, L, channels, bgr, comp, x1, y0);
        if (L.vs == 2) {
            v += enc_component(frame, L, channels, bgr, comp, x0, y1) + enc_component(frame, L, channels, bgr, comp, x1, y1);
            v = (v + 1 + (sx & 1)) >> 2;                                // h2v2: bias 1, 2, 1, 2, ...
        } else {
            v = (v + (sx & 1)) >> 1;                                    // h2v1: bias 0, 1, 0, 1, ...
        }
        d[j] = v - 128;
    }
}

HMM_HD int32_t enc_descale(int32_t x, int n) { return (x + (1 << (n - 1))) >> n; }

// jfdctint.c's butterfly.  first: the row pass (output scaled up by PASS1_BITS); else the column pass.
HMM_HD void enc_fdct_1d(const int32_t* d, int32_t* o, bool first) {
    const int32_t tmp0 = d[0] + d[7], tmp7 = d[0] - d[7], tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
    const int32_t tmp2 = d[2] + d[5], tmp5 = d[2] - d[5], tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
    const int32_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    const int n = first ? 13 - 2 : 13 + 2;
    o[0] = first ? (tmp10 + tmp11) * 4 : enc_descale(tmp10 + tmp11, 2);
    o[4] = first ? (tmp10 - tmp11) * 4 : enc_descale(tmp10 - tmp11, 2);
    int32_t z1 = (tmp12 + tmp13) * 4433;                               // FIX_0_541196100
    o[2] = enc_descale(z1 + tmp13 * 6270, n);                          // FIX_0_765366865
    o[6] = enc_descale(z1 + tmp12 * -15137, n);                        // FIX_1_847759065
    z1 = tmp4 + tmp7;
    int32_t z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int32_t z5 = (z3 + z4) * 9633;                               // FIX_1_175875602
    const int32_t t4 = tmp4 * 2446, t5 = tmp5 * 16819, t6 = tmp6 * 25172, t7 = tmp7 * 12299;
    z1 *= -7373;                                                       // FIX_0_899976223
    z2 *= -20995;                                                      // FIX_2_562915447
    z3 = z3 * -16069 + z5;                                             // FIX_1_961570560
    z4 = z4 * -3196 + z5;                                              // FIX_0_390180644
    o[7] = enc_descale(t4 + z1 + z3, n);
    o[5] = enc_descale(t5 + z2 + z4, n);
    o[3] = enc_descale(t6 + z2 + z3, n);
    o[1] = enc_descale(t7 + z1 + z4, n);
}

HMM_HD int32_t enc_quantise(int32_t v, int32_t q) {
    const int32_t div = q * 8, mag = ((v < 0 ? -v : v) + (div >> 1)) / div;
    return v < 0 ? -mag : mag;
}

// ---- entropy --------------------------------------------------------------------------------------------------------------------
HMM_HD int enc_category(int32_t v) {
    uint32_t m = (uint32_t)(v < 0 ? -v : v);
    int n = 0;
    while (m) {
        ++n;
        m >>= 1;
    }
    return n;
}

struct EncBitCounter {
    uint32_t bits = 0;
    HMM_HD void put(uint32_t, uint32_t len) { bits += len; }
};

// Bits into a zeroed array of 32-bit words, most significant bit first, starting at bit `at`.  The first and the last word a
// block touches may be shared with its neighbours: they are combined with an OR (order-independent); the words between are the
// block's alone.  Words: or_word(index, value) and set_word(index, value).
template <class Words>
struct EncBitWriter {
    Words& words;
    uint64_t acc = 0;
    uint32_t fill;                             // bits of the current word that are decided, the block's predecessors' included
    uint32_t word;
    bool first = true;
    HMM_HD EncBitWriter(Words& w, uint32_t at) : words(w), fill(at & 31), word(at >> 5) {}
    HMM_HD void put(uint32_t code, uint32_t len) {                     // len <= 16
        acc = acc << len | code;
        fill += len;
        if (fill >= 32) {
            fill -= 32;
            const uint32_t v = (uint32_t)(acc >> fill);
            if (first) words.or_word(word, v);
            else words.set_word(word, v);
            first = false;
            ++word;
            acc &= ((uint64_t)1 << fill) - 1;
        }
    }
    HMM_HD void finish() {
        if (fill) words.or_word(word, (uint32_t)(acc << (32 - fill)));
    }
};

// jchuff.c's encode_one_block: zz the block in zigzag order, pred the DC of the component's block before it.
template <class Sink>
HMM_HD void enc_block_bits(const int16_t* zz, int32_t pred, const JpegHuffEnc& dc, const JpegHuffEnc& ac, Sink& s) {
    const int32_t diff = zz[0] - pred;
    int nb = enc_category(diff);
    uint32_t e = dc.e[nb & 15];
    s.put(e & 0xFFFF, e >> 16);
    if (nb) s.put((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << nb) - 1), (uint32_t)nb);
    int run = 0;
#pragma unroll                                                          // static indices: a block held in registers stays there
    for (int k = 1; k < 64; ++k) {
        const int32_t v = zz[k];
        if (v == 0) {
            ++run;
            continue;
        }
        while (run > 15) {
            e = ac.e[0xF0];
            s.put(e & 0xFFFF, e >> 16);
            run -= 16;
        }
        nb = enc_category(v);
        e = ac.e[(run << 4 | nb) & 255];
        s.put(e & 0xFFFF, e >> 16);
        s.put((uint32_t)(v < 0 ? v - 1 : v) & ((1u << nb) - 1), (uint32_t)nb);
        run = 0;
    }
    if (run) {
        e = ac.e[0];
        s.put(e & 0xFFFF, e >> 16);
    }
}

// Byte j of a bitstream kept as 32-bit words, most significant byte first.
HMM_HD uint32_t enc_stream_byte(const uint32_t* words4, uint32_t j) { return (words4[j >> 2] >> (24 - 8 * (j & 3))) & 0xFF; }

// How many of the bytes [first, first + kEncStuffBytes) below `used` are FF; w: the four words that hold them.
HMM_HD uint32_t enc_count_ff(const uint32_t* w, uint32_t first, uint32_t used) {
    uint32_t n = 0;
#pragma unroll
    for (uint32_t j = 0; j < (uint32_t)kEncStuffBytes; ++j) n += (first + j < used && enc_stream_byte(w, j) == 0xFF) ? 1u : 0u;
    return n;
}

// The same bytes to their places behind the header: byte first + j goes to header_bytes + first + j + (FF bytes before it), an FF
// is followed by 00.  Nothing at or beyond `limit` (the slot's size) is written.
HMM_HD void enc_scatter(const uint32_t* w, uint32_t first, uint32_t used, uint32_t ff_before, uint32_t header_bytes,
                        uint8_t* __restrict__ out, uint64_t limit) {
    uint64_t at = (uint64_t)header_bytes + first + ff_before;
#pragma unroll
    for (uint32_t j = 0; j < (uint32_t)kEncStuffBytes; ++j) {
        if (first + j < used) {
            const uint32_t v = enc_stream_byte(w, j);
            if (at < limit) out[at] = (uint8_t)v;
            ++at;
            if (v == 0xFF) {
                if (at < limit) out[at] = 0;
                ++at;
            }
        }
    }
}

}  // namespace hmm
