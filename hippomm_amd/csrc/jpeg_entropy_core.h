// The Huffman (entropy) pass of one baseline JPEG scan, decoded in parallel: the layout of a bitstream slot and the functions
// shared by the host prepare pass (jpeg_host.cpp), the device kernels (jpeg_entropy.hip) and the CPU model that runs the same
// functions thread by thread (tools/jpeg_entropy_model.cpp).
//
// A bitstream slot is what the prepare pass leaves in the caller's pinned memory for one file:
//   [header: 16 int32 | quantisation tables: 3 x 64 uint16 by component, natural order, padded to kJpegQtBytes |
//    4 Huffman tables (EntropyHuff) | the scan's entropy bytes without FF 00 stuffing, zero-padded to kEntropyPad bytes]
//
// The stream is cut into subsequences of kSubBits bits; subsequence i owns the symbols that START inside it.  A decoder state is
// (bit position, block index inside the MCU, zigzag index with 0 = expecting the DC symbol), packed into 64 bits.  Thread t owns
// the contiguous subsequences [t * per, (t + 1) * per).  Entry state 0 is the true one, every other starts as the guess
// (i * kSubBits, 0, 0).  A round decodes every subsequence whose entry state changed, without writing coefficients, and hands
// its exit state to the next subsequence -- inside a thread at once, across threads after a barrier.  Exit states are a
// function of entry states, entry r is right after round r at the latest, so the loop ends within subsequences + 1 rounds at
// the sequential decode.  A speculative decode that meets an invalid code or an index past 63 leaves the sentinel state, which
// decodes to itself; only the write pass, which starts from the fixed point, flags a frame.
//
// After the fixed point a prefix sum over the block counts gives every thread its first block; the write pass decodes once
// more into full-frame coefficients (natural order, zeroed by the caller: a block that straddles two subsequences is written by
// two threads), records DC differences, recomputes every exit state and block count against the recorded ones, and notes the
// bit position at which the last block of the frame ended.  A prefix sum over the DC differences of each thread and a walk over
// the thread's own blocks turn differences into predictors.  finish_block then makes the per-block refusals of the host pass
// (jpeg_host.cpp: block) over ALL blocks and copies the kept ones into the coefficient slot.
#pragma once
#include <stdint.h>
#include <string.h>

#include "jpeg_layout.h"

namespace hmm {

constexpr int kSubBits = 1024;                    // bits per subsequence
constexpr int kEntropyThreads = 256;              // threads per frame on the device
constexpr int kEntropyLook = 9;                   // Huffman lookahead bits, as on the host
constexpr int kEntropyColumnBound = 5800;         // jpeg_host.cpp: kColumnBound
constexpr uint32_t kEntropyMagic = 0x544E454Au;   // "JENT"
constexpr int kEntropyHeaderInts = 16;
constexpr int kEntropyPad = 16;                   // the entropy bytes are zero-padded to a multiple of this
constexpr uint32_t kEntropyMaxBytes = 1u << 27;   // bit positions stay below 2^30

// Header words.
enum { kEhMagic = 0, kEhBytes, kEhComps, kEhHmax, kEhVmax, kEhSelectors, kEhPadded };

struct EntropyHuff {
    uint16_t look[1 << kEntropyLook];             // (code length << 8) | symbol; 0: longer than kEntropyLook bits
    int32_t maxcode[18];                          // by code length; -1: no code of that length
    int32_t valoff[18];
    uint8_t vals[256];
};

constexpr int kEntropyQtOff = kEntropyHeaderInts * 4;
constexpr int kEntropyHuffOff = kEntropyQtOff + kJpegQtBytes;
constexpr int kEntropyDataOff = kEntropyHuffOff + 4 * (int)sizeof(EntropyHuff);
static_assert(sizeof(EntropyHuff) == 1424 && kEntropyDataOff % 16 == 0, "bitstream slot layout");

constexpr uint64_t kStateSentinel = ~0ull;        // exit state of a speculative decode that met corrupt data
constexpr uint32_t kNoEnd = 0xFFFFFFFFu;

__host__ __device__ inline uint64_t state_pack(uint32_t bit, int blk, int zz) { return ((uint64_t)bit << 16) | ((uint64_t)blk << 8) | (uint64_t)zz; }

__host__ __device__ inline int entropy_natural(int k) {
    static constexpr uint8_t tab[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                        41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                        30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return tab[k];
}

// One frame's view for the decoder.  Pointers are LDS, workspace or slot addresses on the device, plain memory in the model.
struct EntropyCtx {
    const uint32_t* words;                        // the entropy bytes as big-endian 32-bit words
    uint32_t nwords;                              // words that may be read (the padded length)
    uint32_t total_bits;
    const EntropyHuff* huff;                      // 4 tables
    uint32_t selectors;                           // component c: DC table in bits [4c, 4c + 2), AC table in bits [4c + 2, 4c + 4)
    int ncomp, hv, bpm;                           // hv: luma blocks per MCU; bpm: blocks per MCU
    uint32_t total_blocks;
    uint32_t nsub, per;                           // subsequences; subsequences per thread
    uint64_t* entry;                              // [nsub]
    uint32_t* count;                              // [nsub] blocks completed by the subsequence
    uint32_t* dirty;                              // [nsub] entry state changed since the subsequence was decoded
    int16_t* coef;                                // [total_blocks][64], natural order
};

__host__ __device__ inline uint32_t entropy_subsequences(uint32_t total_bits) {
    const uint32_t n = (total_bits + kSubBits - 1) / kSubBits;
    return n ? n : 1;
}

__host__ __device__ inline int comp_of(const EntropyCtx& c, int blk) { return blk < c.hv ? 0 : blk - c.hv + 1; }

struct BitReader {
    const uint32_t* w;
    uint32_t nwords, next;
    uint64_t buf;
    int nb;                                       // valid bits: the low nb bits of buf
    __host__ __device__ uint32_t word(uint32_t i) const { return i < nwords ? __builtin_bswap32(w[i]) : 0u; }   // never past the padded end
    __host__ __device__ void seek(const uint32_t* words, uint32_t n, uint32_t bit) {
        w = words;
        nwords = n;
        next = bit >> 5;
        buf = ((uint64_t)word(next) << 32) | word(next + 1);
        next += 2;
        nb = 64 - (int)(bit & 31);
    }
    __host__ __device__ void refill() {           // -> nb >= 33
        if (nb <= 32) {
            buf = (buf << 32) | word(next++);
            nb += 32;
        }
    }
    __host__ __device__ uint32_t peek32() const { return (uint32_t)(buf >> (nb - 32)); }
    __host__ __device__ uint32_t pos() const { return next * 32u - (uint32_t)nb; }
};

struct SubOut {
    uint32_t blocks;                              // blocks completed
    uint32_t ndc;                                 // write pass: DC symbols decoded, and their sum per component
    uint32_t d0, d1, d2;
    uint32_t bad;                                 // write pass: corrupt data
    uint32_t end_bit;                             // write pass: bit position after the frame's last block, else kNoEnd
};

// Decodes the symbols that start in [entry's bit position, end_bit) from `entry` -> exit state.  Write = false: nothing is
// written, corrupt data gives the sentinel.  Write = true: b is the index of the block in progress; coefficients go to c.coef
// (DC as the difference), decoding stops after block total_blocks - 1, corrupt data sets o.bad.
// Every symbol takes at least one bit, so the loop runs at most end_bit - (entry bit) <= kSubBits + 31 times.
template <bool Write>
__host__ __device__ inline uint64_t decode_sub(const EntropyCtx& c, uint64_t entry, uint32_t end_bit, uint32_t b, SubOut& o) {
    o.blocks = o.ndc = o.bad = 0;
    o.d0 = o.d1 = o.d2 = 0;
    o.end_bit = kNoEnd;
    if (entry == kStateSentinel) {
        if (Write) o.bad = 1;
        return kStateSentinel;
    }
    int blk = (int)((entry >> 8) & 255), zz = (int)(entry & 255);
    if (Write && b >= c.total_blocks) return entry;
    BitReader r;
    r.seek(c.words, c.nwords, (uint32_t)(entry >> 16));
    for (int it = 0; it < kSubBits + 32 && r.pos() < end_bit; ++it) {
        r.refill();
        const uint32_t p = r.peek32();
        const int comp = comp_of(c, blk);
        const EntropyHuff& t = c.huff[(c.selectors >> (4 * comp + (zz ? 2 : 0))) & 3];
        int len, sym = -1;
        const uint32_t e = t.look[p >> (32 - kEntropyLook)];
        if (e) {
            len = (int)(e >> 8);
            sym = (int)(e & 255);
        } else {
            for (len = kEntropyLook + 1; len <= 16; ++len) {
                const int32_t code = (int32_t)(p >> (32 - len));
                if (code <= t.maxcode[len]) {
                    const int idx = code + t.valoff[len];
                    if (idx >= 0 && idx < 256) sym = t.vals[idx];
                    break;
                }
            }
        }
        if (sym < 0) {                            // no code of 16 bits or fewer, or a code outside the table
            if (Write) o.bad = 1;
            return kStateSentinel;
        }
        const int s = sym & 15;                   // a DC symbol is its size (<= 15 by the table's construction)
        int v = 0;
        if (s) {
            v = (int)((p << len) >> (32 - s));    // len <= 16, len + s <= 31
            if (v < (1 << (s - 1))) v += 1 - (1 << s);
        }
        bool done = false;
        if (zz == 0) {
            r.nb -= len + s;
            if (Write) {
                c.coef[(size_t)b * 64] = (int16_t)v;
                ++o.ndc;
                o.d0 += comp == 0 ? (uint32_t)v : 0u;          // modulo 2^32 (entropy_dc_walk)
                o.d1 += comp == 1 ? (uint32_t)v : 0u;
                o.d2 += comp == 2 ? (uint32_t)v : 0u;
            }
            zz = 1;
        } else if (s == 0) {
            r.nb -= len;
            if ((sym >> 4) != 15) {
                done = true;                      // EOB
            } else {
                zz += 16;                         // ZRL; past 63 it ends the block, as on the host
                done = zz > 63;
            }
        } else {
            r.nb -= len + s;
            zz += sym >> 4;
            if (zz > 63) {
                if (Write) o.bad = 1;
                return kStateSentinel;
            }
            if (Write) c.coef[(size_t)b * 64 + entropy_natural(zz)] = (int16_t)v;
            done = ++zz > 63;
        }
        if (done) {
            zz = 0;
            blk = blk + 1 == c.bpm ? 0 : blk + 1;
            ++o.blocks;
            if (Write && ++b == c.total_blocks) {
                o.end_bit = r.pos();
                break;
            }
        }
    }
    return state_pack(r.pos(), blk, zz);
}

__host__ __device__ inline void entropy_range(const EntropyCtx& c, uint32_t t, uint32_t& lo, uint32_t& hi) {
    lo = t * c.per < c.nsub ? t * c.per : c.nsub;
    hi = lo + c.per < c.nsub ? lo + c.per : c.nsub;
}

__host__ __device__ inline uint32_t entropy_sub_end(const EntropyCtx& c, uint32_t i) {
    const uint32_t e = (i + 1) * (uint32_t)kSubBits;
    return e < c.total_bits ? e : c.total_bits;
}

// ---- the phases; a barrier stands between two of them ------------------------------------------------------------------------

__host__ __device__ inline void entropy_init(const EntropyCtx& c, uint32_t t, uint64_t* boundary) {
    uint32_t lo, hi;
    entropy_range(c, t, lo, hi);
    for (uint32_t i = lo; i < hi; ++i) {
        c.entry[i] = i ? state_pack(i * (uint32_t)kSubBits, 0, 0) : 0;
        c.dirty[i] = 1;
    }
    boundary[t] = kStateSentinel;
}

// Decodes the thread's subsequences whose entry changed; boundary[t] keeps the exit state of its last one.
__host__ __device__ inline void entropy_round(const EntropyCtx& c, uint32_t t, uint64_t* boundary) {
    uint32_t lo, hi;
    entropy_range(c, t, lo, hi);
    for (uint32_t i = lo; i < hi; ++i) {
        if (!c.dirty[i]) continue;
        SubOut o;
        const uint64_t ex = decode_sub<false>(c, c.entry[i], entropy_sub_end(c, i), 0, o);
        c.count[i] = o.blocks;
        c.dirty[i] = 0;
        if (i + 1 < hi) {
            if (c.entry[i + 1] != ex) {
                c.entry[i + 1] = ex;
                c.dirty[i + 1] = 1;
            }
        } else {
            boundary[t] = ex;
        }
    }
}

// Takes the previous thread's exit state as this thread's first entry state -> did it change?
__host__ __device__ inline bool entropy_sync(const EntropyCtx& c, uint32_t t, const uint64_t* boundary) {
    uint32_t lo, hi;
    entropy_range(c, t, lo, hi);
    if (t == 0 || lo >= hi || c.entry[lo] == boundary[t - 1]) return false;
    c.entry[lo] = boundary[t - 1];
    c.dirty[lo] = 1;
    return true;
}

__host__ __device__ inline uint32_t entropy_thread_blocks(const EntropyCtx& c, uint32_t t) {
    uint32_t lo, hi, sum = 0;
    entropy_range(c, t, lo, hi);
    for (uint32_t i = lo; i < hi; ++i) sum += c.count[i];
    return sum;
}

struct ThreadOut {
    uint32_t dc_first, ndc;                       // the thread decoded the DC symbols of blocks [dc_first, dc_first + ndc)
    uint32_t d0, d1, d2;                           // their sums per component
    uint32_t bad;
    uint32_t end_bit;
};

// The write pass of thread t, whose first subsequence starts inside block `base`.
__host__ __device__ inline void entropy_write(const EntropyCtx& c, uint32_t t, uint32_t base, ThreadOut& out) {
    uint32_t lo, hi;
    entropy_range(c, t, lo, hi);
    out.dc_first = base;
    out.ndc = out.bad = 0;
    out.d0 = out.d1 = out.d2 = 0;
    out.end_bit = kNoEnd;
    uint32_t b = base;
    for (uint32_t i = lo; i < hi; ++i) {
        const uint64_t en = c.entry[i];
        if (i == lo && en != kStateSentinel && (en & 255) != 0) out.dc_first = base + 1;
        if (b >= c.total_blocks) break;           // data after the frame's last block: the end check refuses it
        SubOut o;
        const uint64_t ex = decode_sub<true>(c, en, entropy_sub_end(c, i), b, o);
        out.ndc += o.ndc;
        out.d0 += o.d0;
        out.d1 += o.d1;
        out.d2 += o.d2;
        out.bad |= o.bad;
        b += o.blocks;
        if (o.end_bit != kNoEnd) {
            out.end_bit = o.end_bit;
            break;
        }
        if (o.bad) break;
        // self-check: the fixed point must reproduce itself
        if (o.blocks != c.count[i] || (i + 1 < c.nsub && c.entry[i + 1] != ex)) {
            out.bad = 1;
            break;
        }
    }
}

// DC differences -> predictors for the blocks whose DC symbol this thread decoded; run0..2 are the predictors before them.
// -> a predictor left int16.  Sums are taken modulo 2^32: up to the first predictor outside int16 they are exact.
__host__ __device__ inline uint32_t entropy_dc_walk(const EntropyCtx& c, const ThreadOut& th, int32_t run0, int32_t run1, int32_t run2) {
    uint32_t bad = 0;
    uint32_t blk = th.dc_first % (uint32_t)c.bpm;
    for (uint32_t k = 0; k < th.ndc; ++k) {
        const uint32_t b = th.dc_first + k;
        if (b >= c.total_blocks) return 1;        // cannot happen at the fixed point; keeps every access inside the frame
        const int comp = comp_of(c, (int)blk);
        const int32_t d = c.coef[(size_t)b * 64];
        int32_t p;
        if (comp == 0) p = run0 = (int32_t)((uint32_t)run0 + (uint32_t)d);
        else if (comp == 1) p = run1 = (int32_t)((uint32_t)run1 + (uint32_t)d);
        else p = run2 = (int32_t)((uint32_t)run2 + (uint32_t)d);
        if (p < -32768 || p > 32767) bad = 1;
        c.coef[(size_t)b * 64] = (int16_t)p;
        blk = blk + 1 == (uint32_t)c.bpm ? 0 : blk + 1;
    }
    return bad;
}

// The frame-level refusals of the host pass: a bit taken from past the end of the data, 8 or more unused bits, a frame that
// never reached its last block.
__host__ __device__ inline bool entropy_end_ok(uint32_t end_bit, uint32_t total_bits) {
    return end_bit != kNoEnd && end_bit <= total_bits && total_bits - end_bit < 8;
}

struct Row8 {
    uint32_t x, y, z, w;                          // 8 int16 or uint16
};
__host__ __device__ inline int row_i16(const Row8& r, int k) {
    const uint32_t u = k < 2 ? r.x : k < 4 ? r.y : k < 6 ? r.z : r.w;
    return (int)(int16_t)(uint16_t)(u >> (16 * (k & 1)));
}
__host__ __device__ inline int row_u16(const Row8& r, int k) {
    const uint32_t u = k < 2 ? r.x : k < 4 ? r.y : k < 6 ? r.z : r.w;
    return (int)(uint16_t)(u >> (16 * (k & 1)));
}

// Block b (scan order) of a frame: the host's refusals on dequantised magnitudes, and the copy into the slot when the window
// keeps the block.  coef: the frame's coefficients with DC predictors in place; qt: 3 x 64 uint16.  -> refused.
__host__ __device__ inline bool finish_block(const int16_t* coef, const uint16_t* qt, const JpegLayout& L, int mcux, int hv, int bpm,
                                             uint32_t b, uint8_t* slot) {
    const uint32_t m = b / (uint32_t)bpm;
    const int j = (int)(b - m * (uint32_t)bpm);
    const int comp = j < hv ? 0 : j - hv + 1;
    const int hs = comp == 0 ? L.rx : 1, vs = comp == 0 ? L.ry : 1;
    const int u = comp == 0 ? j % hs : 0, v = comp == 0 ? j / hs : 0;
    const int bx = (int)(m % (uint32_t)mcux) * hs + u - L.bx0[comp], by = (int)(m / (uint32_t)mcux) * vs + v - L.by0[comp];
    const bool kept = bx >= 0 && bx < L.nbx[comp] && by >= 0 && by < L.nby[comp];
    const Row8* src = reinterpret_cast<const Row8*>(coef + (size_t)b * 64);
    const Row8* q = reinterpret_cast<const Row8*>(qt + 64 * comp);
    Row8* dst = reinterpret_cast<Row8*>(slot + kJpegQtBytes + (kept ? (L.block_off[comp] + (int64_t)by * L.nbx[comp] + bx) : 0) * kJpegBlockBytes);
    int col[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool bad = false;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const Row8 row = src[r], qr = q[r];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int val = row_i16(row, k);
            const int mag = (val < 0 ? -val : val) * row_u16(qr, k);
            bad |= mag > 32767;
            col[k] += mag;
        }
        if (kept) dst[r] = row;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) bad |= col[k] > kEntropyColumnBound;
    return bad;
}

// Workspace of one frame: [coefficients | entry | count | dirty], each part 256-byte aligned.
struct EntropyWorkspace {
    size_t coef_bytes, entry_off, count_off, dirty_off, frame_bytes;
    uint32_t max_sub;
};
inline size_t entropy_up256(size_t x) { return (x + 255) / 256 * 256; }
inline EntropyWorkspace entropy_workspace(uint32_t total_blocks, size_t max_entropy_bytes) {
    EntropyWorkspace w;
    w.max_sub = (uint32_t)((max_entropy_bytes * 8 + kSubBits - 1) / kSubBits) + 1;
    w.coef_bytes = entropy_up256((size_t)total_blocks * kJpegBlockBytes);
    w.entry_off = w.coef_bytes;
    w.count_off = w.entry_off + entropy_up256((size_t)w.max_sub * 8);
    w.dirty_off = w.count_off + entropy_up256((size_t)w.max_sub * 4);
    w.frame_bytes = w.dirty_off + entropy_up256((size_t)w.max_sub * 4);
    return w;
}

inline uint32_t entropy_total_blocks(int W, int H, int ncomp, int hmax, int vmax) {
    if (ncomp == 1) return (uint32_t)jpeg_cdiv(W, 8) * (uint32_t)jpeg_cdiv(H, 8);
    return (uint32_t)jpeg_cdiv(W, 8 * hmax) * (uint32_t)jpeg_cdiv(H, 8 * vmax) * (uint32_t)(hmax * vmax + 2);
}

}  // namespace hmm
