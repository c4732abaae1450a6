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

}  // namespace hmm
