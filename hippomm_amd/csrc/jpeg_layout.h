// Where the coefficient blocks of one baseline JPEG frame live in a coefficient slot and in the device workspace: shared by the
// host entropy decoder (jpeg_host.cpp) and the reconstruction kernels (jpeg.hip), so both sides agree by construction.
//
// A slot is [quantisation tables: 3 x 64 uint16, natural order | pad to kJpegQtBytes | coefficient blocks].  Component c keeps the
// rectangle of blocks [bx0, bx0 + nbx) x [by0, by0 + nby) of its block grid, row-major, 64 int16 per block in natural order: the
// blocks under the output window plus the one-sample halo that fancy upsampling reads.  The workspace holds the same rectangles
// as u8 sample planes (nbx * 8 wide, nby * 8 high) per frame.
#pragma once
#include <stdint.h>

namespace hmm {

constexpr int kJpegQtBytes = 512;             // 3 * 64 * 2 = 384, padded
constexpr int kJpegBlockBytes = 64 * 2;

struct JpegLayout {
    int32_t ncomp;                            // 1 (grey) or 3 (YCbCr)
    int32_t rx, ry;                           // chroma upsampling ratio: luma sampling factors (1 or 2) for 3 components
    int32_t fancy;                            // libjpeg-turbo's triangle filter (chroma downsampled width > 2), else replication
    int32_t x0, y0, w, h;                     // output window in frame pixels
    int32_t cw[3], ch[3];                     // component size in samples (libjpeg's downsampled_width / _height)
    int32_t bx0[3], by0[3], nbx[3], nby[3];   // stored block rectangle of each component
    int64_t block_off[4];                     // first block of component c in the slot's block list; [ncomp] = blocks per frame
    int64_t plane_off[4];                     // byte offset of component c's plane in a frame's workspace; [ncomp] = bytes per frame
    int64_t slot_bytes;                       // kJpegQtBytes + blocks * kJpegBlockBytes, a multiple of 256
};

__host__ __device__ inline int jpeg_cdiv(int a, int b) { return (a + b - 1) / b; }

// geometry: W x H frame, ncomp components, luma sampling (hmax, vmax) (1 x 1 for grey).  Window [x0, x0 + w) x [y0, y0 + h) must
// lie inside the frame.  -> false for a bad window.
inline bool jpeg_layout(int W, int H, int ncomp, int hmax, int vmax, int x0, int y0, int w, int h, JpegLayout* L) {
    if (W < 1 || H < 1 || (ncomp != 1 && ncomp != 3) || w < 1 || h < 1 || x0 < 0 || y0 < 0 || x0 + w > W || y0 + h > H) return false;
    if (ncomp == 1) hmax = vmax = 1;
    *L = JpegLayout{};
    L->ncomp = ncomp;
    L->rx = hmax;
    L->ry = vmax;
    L->x0 = x0;
    L->y0 = y0;
    L->w = w;
    L->h = h;
    const int mcux = jpeg_cdiv(W, 8 * hmax), mcuy = jpeg_cdiv(H, 8 * vmax);
    int64_t blocks = 0, bytes = 0;
    for (int c = 0; c < ncomp; ++c) {
        const int hc = c == 0 ? hmax : 1, vc = c == 0 ? vmax : 1;
        L->cw[c] = jpeg_cdiv(W * hc, hmax);
        L->ch[c] = jpeg_cdiv(H * vc, vmax);
        const int gw = ncomp == 1 ? jpeg_cdiv(W, 8) : mcux * hc, gh = ncomp == 1 ? jpeg_cdiv(H, 8) : mcuy * vc;
        int sx0 = x0, sx1 = x0 + w, sy0 = y0, sy1 = y0 + h;          // samples of component c the window reads
        if (c > 0) {
            L->fancy = L->cw[c] > 2;
            const int halo = L->fancy ? 1 : 0;
            if (hmax == 2) {
                sx0 = (x0 >> 1) - halo;
                sx1 = ((x0 + w - 1) >> 1) + 1 + halo;
            }
            if (vmax == 2) {
                sy0 = (y0 >> 1) - halo;
                sy1 = ((y0 + h - 1) >> 1) + 1 + halo;
            }
            sx0 = sx0 < 0 ? 0 : sx0;
            sy0 = sy0 < 0 ? 0 : sy0;
            sx1 = sx1 > L->cw[c] ? L->cw[c] : sx1;
            sy1 = sy1 > L->ch[c] ? L->ch[c] : sy1;
        }
        L->bx0[c] = sx0 / 8;
        L->by0[c] = sy0 / 8;
        L->nbx[c] = jpeg_cdiv(sx1, 8) - L->bx0[c];
        L->nby[c] = jpeg_cdiv(sy1, 8) - L->by0[c];
        if (L->bx0[c] + L->nbx[c] > gw || L->by0[c] + L->nby[c] > gh) return false;
        L->block_off[c] = blocks;
        L->plane_off[c] = bytes;
        blocks += (int64_t)L->nbx[c] * L->nby[c];
        bytes += (int64_t)L->nbx[c] * L->nby[c] * 64;
    }
    L->block_off[ncomp] = blocks;
    L->plane_off[ncomp] = bytes;
    L->slot_bytes = ((kJpegQtBytes + blocks * kJpegBlockBytes) + 255) / 256 * 256;
    return true;
}

// ---- encoding (jpeg_encode.hip, jpeg_encode_host.cpp, tools/jpeg_encode_model.cpp) ---------------------------------------------
// The tables of a baseline file written with libjpeg's defaults: the example quantisation tables of the standard's Annex K
// (natural order, scaled by jpeg_quality_scaling) and its typical Huffman tables (counts per code length, then the symbols).
constexpr uint8_t kJpegStdLumaQ[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40, 57,
                                       69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55, 64,
                                       81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr uint8_t kJpegStdChromaQ[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                         99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                         99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
constexpr uint8_t kJpegZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                     41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                     30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};   // natural index of zigzag k

struct JpegStdHuff {
    uint8_t bits[16];                         // codes of length 1..16
    uint8_t nvals;
    uint8_t vals[162];
};
constexpr JpegStdHuff kJpegStdDcLuma = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr JpegStdHuff kJpegStdDcChroma = {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr JpegStdHuff kJpegStdAcLuma = {
    {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
    162,
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
     0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
     0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
     0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
     0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
     0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
     0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};
constexpr JpegStdHuff kJpegStdAcChroma = {
    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77},
    162,
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
     0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
     0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
     0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
     0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
     0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
     0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// A symbol's code as the encoder looks it up: code | length << 16; 0 for a symbol the table does not have.
struct JpegHuffEnc {
    uint32_t e[256];
};
constexpr JpegHuffEnc jpeg_huff_enc(const JpegStdHuff& t) {             // Annex C: codes in order of length, then of listing
    JpegHuffEnc out{};
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < t.bits[len - 1]; ++i, ++k, ++code) out.e[t.vals[k]] = code | (uint32_t)len << 16;
        code <<= 1;
    }
    return out;
}

// Bits of one block at most (the proof of hmm_jpeg_encode_bound): the DC symbol is a code of at most 11 bits (the longest in the
// two DC tables is 11) and at most 11 amplitude bits; each of the 63 AC positions is covered by exactly one symbol -- a
// coefficient's run/size symbol covers its zeros and itself, a ZRL covers 16 zeros, EOB the rest -- and a symbol costs at most 16
// code bits plus 10 amplitude bits: 22 + 63 * 26.  The categories (DC difference <= 11, AC <= 10) hold for 8-bit input: a sample
// is in [-128, 127] after the level shift, |DC| <= 1024 so |difference| <= 2047 at quantiser 1; the AC basis function with the
// largest absolute sum is (4, 0) / (0, 4) / (4, 4), whose coefficient is at most (32 * 128 + 32 * 127) / 8 = 1020, and
// jfdctint.c's rounding adds less than 3.
constexpr uint32_t kJpegMaxBlockBits = 22 + 63 * 26;
constexpr uint32_t kJpegHeaderColor = 623, kJpegHeaderGrey = 328;     // FF D8 .. SOS as hmm_jpeg_encode_header writes them

// One frame to encode: W x H, ncomp 1 (grey) or 3 (YCbCr), luma sampling (hs, vs) in {(1,1), (2,1), (2,2)}.  The scan is the
// frame's MCUs row by row; a colour MCU is hs * vs luma blocks (row by row), then Cb, then Cr; a grey MCU is one block.
struct JpegEncLayout {
    int32_t w, h, ncomp, hs, vs;
    int32_t mcux, mcuy, bpm;                  // MCUs across and down, blocks per MCU
    int32_t wib, hib;                         // luma blocks that exist: ceil(w / 8) x ceil(h / 8); the rest of an MCU is dummies
    int32_t cw, ch;                           // chroma samples that exist: ceil(w / hs) x ceil(h / vs)
    uint32_t blocks;                          // per frame
    uint32_t header_bytes;
    uint32_t bit_bytes;                       // capacity of the unstuffed bitstream of one frame: a multiple of 16
};

inline bool jpeg_enc_layout(int w, int h, int ncomp, int hs, int vs, JpegEncLayout* L) {
    if (w < 1 || h < 1 || w > 65535 || h > 65535 || (ncomp != 1 && ncomp != 3)) return false;
    if (ncomp == 1) hs = vs = 1;
    if (!((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2))) return false;
    *L = JpegEncLayout{};
    L->w = w, L->h = h, L->ncomp = ncomp, L->hs = hs, L->vs = vs;
    L->mcux = jpeg_cdiv(w, 8 * hs), L->mcuy = jpeg_cdiv(h, 8 * vs);
    L->bpm = ncomp == 1 ? 1 : hs * vs + 2;
    L->wib = jpeg_cdiv(w, 8), L->hib = jpeg_cdiv(h, 8);
    L->cw = jpeg_cdiv(w, hs), L->ch = jpeg_cdiv(h, vs);
    const uint64_t blocks = (uint64_t)L->mcux * L->mcuy * L->bpm;
    if (blocks * kJpegMaxBlockBits + 7 >= (1ull << 32)) return false;   // bit offsets are 32-bit
    L->blocks = (uint32_t)blocks;
    L->header_bytes = ncomp == 3 ? kJpegHeaderColor : kJpegHeaderGrey;
    L->bit_bytes = (uint32_t)((blocks * kJpegMaxBlockBits + 7) / 8 + 15) / 16 * 16;
    return true;
}

}  // namespace hmm
