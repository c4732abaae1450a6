// Host half of the baseline JPEG decoder (no GPU call in this file): marker parsing and the Huffman (entropy) pass into dense
// int16 coefficient blocks.  Dequantisation, IDCT, upsampling and colour conversion run on the GPU (jpeg.hip).
//
// The decoder takes a narrow class of files -- 8-bit Huffman sequential (SOF0 / SOF1), one interleaved scan of grey or YCbCr
// with luma sampling 1x1, 2x1 or 2x2 and chroma 1x1, restart intervals allowed -- and answers HMM_JPEG_UNSUPPORTED for
// everything else and for every anomaly (truncation, a bad code, a restart marker out of sequence, extraneous bytes, a missing
// EOI, a coefficient past position 63, dequantised coefficients too large for the IDCT's int16 stages: see kColumnBound).
// libjpeg would warn, resync, or carry on with data it made up in these cases; here the caller hands such a file to Pillow unchanged, so its pixels and errors stay
// Pillow's.  Every read is bounds-checked and every loop is bounded by the frame's MCU count: no input can crash or hang it.
//
// Called through ctypes, one frame per call, with the interpreter lock released: the package's decode thread pool runs it.
#include "hmm_common.h"
#include "jpeg_layout.h"
#include "jpeg_entropy_core.h"

#include <cstring>

namespace {

using hmm::JpegLayout;

constexpr int kLook = 9;                          // Huffman lookahead bits

const uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                              41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                              30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Huff {
    bool defined = false;
    uint8_t bits[17];
    uint8_t vals[256];
    int32_t maxcode[18];
    int32_t valoff[17];
    uint16_t look[1 << kLook];                    // (code length << 8) | symbol; 0: longer than kLook bits
    int32_t fast_ac[1 << kLook];                  // AC: (value << 16) | (run << 8) | (code + value bits); 0: not in kLook bits
};

// libjpeg's jpeg_make_d_derived_tbl, with the same refusals (too many symbols, an overfull code, a DC symbol above 15).
bool derive(Huff& t, bool dc) {
    uint8_t size[257];
    uint32_t code_of[257];
    int p = 0;
    for (int l = 1; l <= 16; ++l)
        for (int i = 0; i < t.bits[l]; ++i) {
            if (p >= 256) return false;
            size[p++] = (uint8_t)l;
        }
    size[p] = 0;
    const int total = p;
    uint32_t code = 0;
    int si = size[0];
    p = 0;
    while (size[p]) {
        while (size[p] == si) {
            code_of[p++] = code;
            ++code;
        }
        if (code >= (1u << si)) return false;
        code <<= 1;
        ++si;
    }
    p = 0;
    for (int l = 1; l <= 16; ++l) {
        if (t.bits[l]) {
            t.valoff[l] = p - (int32_t)code_of[p];
            p += t.bits[l];
            t.maxcode[l] = (int32_t)code_of[p - 1];
        } else {
            t.maxcode[l] = -1;
        }
    }
    t.maxcode[17] = 0x7FFFFFFF;
    if (dc)
        for (int i = 0; i < total; ++i)
            if (t.vals[i] > 15) return false;
    memset(t.look, 0, sizeof(t.look));
    memset(t.fast_ac, 0, sizeof(t.fast_ac));
    p = 0;
    for (int l = 1; l <= kLook; ++l)
        for (int i = 0; i < t.bits[l]; ++i, ++p) {
            const int lo = (int)(code_of[p] << (kLook - l)), span = 1 << (kLook - l);
            for (int j = 0; j < span; ++j) t.look[lo + j] = (uint16_t)((l << 8) | t.vals[p]);
            const int r = t.vals[p] >> 4, s = t.vals[p] & 15;
            if (dc || s == 0 || l + s > kLook) continue;
            for (int j = 0; j < span; ++j) {
                int v = ((lo + j) >> (kLook - l - s)) & ((1 << s) - 1);
                if (v < (1 << (s - 1))) v += 1 - (1 << s);
                t.fast_ac[lo + j] = (int32_t)((uint32_t)(v & 0xFFFF) << 16) | (r << 8) | (l + s);
            }
        }
    return true;
}

struct Frame {
    int W = 0, H = 0, ncomp = 0, hmax = 1, vmax = 1, restart = 0;
    int id[3], hs[3], vs[3], tq[3], td[3], ta[3];
    bool qdef[4] = {false, false, false, false};
    uint16_t q[4][64];                            // natural order
    Huff dc[4], ac[4];
    size_t scan = 0;                              // first byte of the entropy-coded data
};

inline int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// Markers up to the first scan.  -> false for anything outside the supported class.
bool parse(const uint8_t* d, size_t n, Frame& f) {
    if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) return false;
    size_t pos = 2;
    bool sof = false;
    for (;;) {
        if (pos + 1 >= n || d[pos] != 0xFF) return false;  // extraneous bytes: libjpeg warns and skips, Pillow's route decides
        while (pos + 1 < n && d[pos + 1] == 0xFF) ++pos;    // fill bytes
        if (pos + 3 >= n) return false;
        const int m = d[pos + 1];
        if (m == 0xD8 || m == 0xD9 || m == 0x01 || (m >= 0xD0 && m <= 0xD7) || m == 0x00) return false;
        const int len = be16(d + pos + 2);
        if (len < 2 || pos + 2 + (size_t)len > n) return false;
        const uint8_t* s = d + pos + 4;
        const int body = len - 2;
        if (m == 0xC0 || m == 0xC1) {
            if (sof || body < 6) return false;
            sof = true;
            f.H = be16(s + 1);
            f.W = be16(s + 3);
            f.ncomp = s[5];
            if (s[0] != 8 || f.H == 0 || f.W == 0 || (f.ncomp != 1 && f.ncomp != 3) || body != 6 + 3 * f.ncomp) return false;
            for (int c = 0; c < f.ncomp; ++c) {
                f.id[c] = s[6 + 3 * c];
                f.hs[c] = s[7 + 3 * c] >> 4;
                f.vs[c] = s[7 + 3 * c] & 15;
                f.tq[c] = s[8 + 3 * c];
                if (f.hs[c] < 1 || f.hs[c] > 4 || f.vs[c] < 1 || f.vs[c] > 4 || f.tq[c] > 3) return false;
                for (int e = 0; e < c; ++e)
                    if (f.id[e] == f.id[c]) return false;
            }
            if (f.ncomp == 3) {
                if (f.id[0] == 'R' && f.id[1] == 'G' && f.id[2] == 'B') return false;     // libjpeg: RGB, not YCbCr
                const bool luma_ok = (f.hs[0] == 1 && f.vs[0] == 1) || (f.hs[0] == 2 && f.vs[0] == 1) || (f.hs[0] == 2 && f.vs[0] == 2);
                if (!luma_ok || f.hs[1] != 1 || f.vs[1] != 1 || f.hs[2] != 1 || f.vs[2] != 1) return false;
                f.hmax = f.hs[0];
                f.vmax = f.vs[0];
            }                                                                               // grey: one block per MCU
        } else if (m == 0xC4) {
            int i = 0;
            while (i < body) {
                if (i + 17 > body) return false;
                const int tc = s[i] >> 4, th = s[i] & 15;
                if (tc > 1 || th > 3) return false;
                Huff& t = tc ? f.ac[th] : f.dc[th];
                int count = 0;
                t.bits[0] = 0;
                for (int l = 1; l <= 16; ++l) count += (t.bits[l] = s[i + l]);
                if (count > 256 || i + 17 + count > body) return false;
                memcpy(t.vals, s + i + 17, count);
                if (!derive(t, tc == 0)) return false;
                t.defined = true;
                i += 17 + count;
            }
        } else if (m == 0xDB) {
            int i = 0;
            while (i < body) {
                const int pq = s[i] >> 4, tq = s[i] & 15;
                if (pq > 1 || tq > 3 || i + 1 + 64 * (pq + 1) > body) return false;
                for (int k = 0; k < 64; ++k) {
                    const int v = pq ? be16(s + i + 1 + 2 * k) : s[i + 1 + k];
                    if (v > 32767) return false;           // a SIMD libjpeg-turbo keeps quantisers in int16
                    f.q[tq][kNatural[k]] = (uint16_t)v;
                }
                f.qdef[tq] = true;
                i += 1 + 64 * (pq + 1);
            }
        } else if (m == 0xDD) {
            if (body != 2) return false;
            f.restart = be16(s);
        } else if (m == 0xDA) {
            if (!sof || body < 1) return false;
            const int ns = s[0];
            if (ns != f.ncomp || body != 4 + 2 * ns) return false;
            for (int c = 0; c < ns; ++c) {
                if (s[1 + 2 * c] != f.id[c]) return false;                                  // scan order = frame order
                f.td[c] = s[2 + 2 * c] >> 4;
                f.ta[c] = s[2 + 2 * c] & 15;
                if (f.td[c] > 3 || f.ta[c] > 3 || !f.dc[f.td[c]].defined || !f.ac[f.ta[c]].defined || !f.qdef[f.tq[c]]) return false;
            }
            const uint8_t* e = s + 1 + 2 * ns;
            if (e[0] != 0 || e[1] != 63 || e[2] != 0) return false;                          // Ss, Se, Ah/Al of a sequential scan
            f.scan = pos + 2 + len;
            return true;
        } else if (m == 0xEE) {
            if (body >= 5 && memcmp(s, "Adobe", 5) == 0) return false;                       // colour transform: not ours
        } else if ((m >= 0xE0 && m <= 0xEF) || m == 0xFE) {
            // APPn, COM: skipped
        } else {
            return false;                                                                   // SOF2+, DAC, DNL, DHP, EXP, JPGn, ...
        }
        pos += 2 + len;
    }
}

struct Bits {
    const uint8_t* d;
    size_t n, pos;
    uint64_t buf = 0;
    int nbits = 0, npad = 0;                      // npad: zero bits supplied past a marker or the end of the data
    bool marker = false;

    void fill() {
        while (nbits <= 56) {
            uint32_t b = 0;
            if (marker || pos >= n) {
                marker = true;
                npad += 8;
            } else if ((b = d[pos]) == 0xFF) {
                if (pos + 1 < n && d[pos + 1] == 0) {
                    pos += 2;
                } else {
                    b = 0;                         // a marker: stay on it
                    marker = true;
                    npad += 8;
                }
            } else {
                ++pos;
            }
            buf = (buf << 8) | b;
            nbits += 8;
        }
    }
    uint32_t peek(int k) const { return (uint32_t)(buf >> (nbits - k)) & ((1u << k) - 1); }
    int symbol(const Huff& t) {                   // needs nbits >= 16
        const uint32_t e = t.look[peek(kLook)];
        if (e) {
            nbits -= e >> 8;
            return e & 255;
        }
        for (int l = kLook + 1; l <= 16; ++l) {
            const int32_t code = (int32_t)peek(l);
            if (code <= t.maxcode[l]) {
                nbits -= l;
                const int idx = code + t.valoff[l];
                return (idx >= 0 && idx < 256) ? t.vals[idx] : -1;
            }
        }
        return -1;                                // no code of 16 bits or fewer: corrupt data
    }
    int value(int s) {                            // s <= 15 extra bits, sign-extended (HUFF_EXTEND); needs nbits >= s
        if (s == 0) return 0;
        int v = (int)peek(s);
        nbits -= s;
        return v < (1 << (s - 1)) ? v + 1 - (1 << s) : v;
    }
    // After the last MCU of an interval: no whole unused byte before the marker, no bit taken from past it, and the marker
    // is `want`.  Then step over it.
    bool marker_is(int want) {
        if (nbits < npad || nbits - npad >= 8) return false;
        if (pos + 1 >= n || d[pos] != 0xFF || d[pos + 1] != want) return false;
        pos += 2;
        buf = 0;
        nbits = npad = 0;
        marker = false;
        return true;
    }
};

// One block: DC difference and AC run / values into blk (natural order; zeroed here) or, blk = nullptr, only consumed.
// -> false for corrupt data or a coefficient the device arithmetic would not reproduce (see the top of the file).
// The dequantised magnitudes of each column must sum to at most kColumnBound: then every value of the IDCT's first pass fits
// int16 (the largest islow gain is 4 x 1.387), where libjpeg-turbo's SIMD IDCT keeps it.  A file from an 8-bit encoder stays
// far below (an orthonormal block has sum |F| <= sqrt(8) * 1024 per column, plus 4 q of rounding); corrupt data may not.
constexpr int kColumnBound = 5800;

inline bool block(Bits& b, const Huff& dc, const Huff& ac, const uint16_t* q, int& pred, int16_t* blk) {
    if (blk) memset(blk, 0, 64 * sizeof(int16_t));
    int col[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (b.nbits < 32) b.fill();
    const int s = b.symbol(dc);
    if (s < 0) return false;
    pred += b.value(s);
    if (pred < -32768 || pred > 32767 || (pred < 0 ? -pred : pred) * (int)q[0] > 32767) return false;
    if (blk) blk[0] = (int16_t)pred;
    col[0] = (pred < 0 ? -pred : pred) * (int)q[0];
    for (int k = 1; k < 64;) {
        if (b.nbits < 32) b.fill();
        const int32_t fe = ac.fast_ac[b.peek(kLook)];
        int v, r;
        if (fe) {
            r = (fe >> 8) & 15;
            v = fe >> 16;
            b.nbits -= fe & 255;
        } else {
            const int sym = b.symbol(ac);
            if (sym < 0) return false;
            r = sym >> 4;
            const int sz = sym & 15;
            if (sz == 0) {
                if (r != 15) break;               // EOB
                k += 16;                          // ZRL
                continue;
            }
            v = b.value(sz);
        }
        k += r;
        if (k > 63) return false;                 // libjpeg would write it to position 63
        const int nat = kNatural[k];
        const int mag = (v < 0 ? -v : v) * (int)q[nat];
        if (mag > 32767) return false;
        col[nat & 7] += mag;
        if (blk) blk[nat] = (int16_t)v;
        ++k;
    }
    for (int t = 0; t < 8; ++t)
        if (col[t] > kColumnBound) return false;
    return true;
}

}  // namespace

extern "C" int hmm_jpeg_parse(const uint8_t* data, size_t n, int32_t* geometry) {
    HMM_REQUIRE(data && geometry, HMM_E_INVALID, "jpeg_parse: null pointer");
    Frame f;
    if (!parse(data, n, f)) return HMM_JPEG_UNSUPPORTED;
    const int32_t g[HMM_JPEG_GEOMETRY_INTS] = {f.W, f.H, f.ncomp, f.ncomp == 3 ? f.hmax : 1, f.ncomp == 3 ? f.vmax : 1, f.restart};
    memcpy(geometry, g, sizeof(g));
    return HMM_JPEG_DECODED;
}

extern "C" int64_t hmm_jpeg_slot_bytes(const int32_t* geometry, int x0, int y0, int w, int h) {
    JpegLayout L;
    if (!geometry || !hmm::jpeg_layout(geometry[0], geometry[1], geometry[2], geometry[3], geometry[4], x0, y0, w, h, &L)) return 0;
    return L.slot_bytes;
}

extern "C" int hmm_jpeg_decode_coefs(const uint8_t* data, size_t n, const int32_t* geometry, int x0, int y0, int w, int h,
                                     void* slot, size_t slot_bytes) {
    HMM_REQUIRE(data && geometry && slot, HMM_E_INVALID, "jpeg_decode_coefs: null pointer");
    JpegLayout L;
    HMM_REQUIRE(hmm::jpeg_layout(geometry[0], geometry[1], geometry[2], geometry[3], geometry[4], x0, y0, w, h, &L), HMM_E_INVALID,
                "jpeg_decode_coefs: window (%d, %d, %d, %d) outside the %d x %d frame", x0, y0, w, h, geometry[0], geometry[1]);
    HMM_REQUIRE(slot_bytes >= (size_t)L.slot_bytes, HMM_E_WORKSPACE, "jpeg_decode_coefs: slot of %zu bytes, %lld needed", slot_bytes,
                (long long)L.slot_bytes);
    Frame f;
    if (!parse(data, n, f)) return HMM_JPEG_UNSUPPORTED;
    const int hmax = f.ncomp == 3 ? f.hmax : 1, vmax = f.ncomp == 3 ? f.vmax : 1;
    if (f.W != geometry[0] || f.H != geometry[1] || f.ncomp != geometry[2] || hmax != geometry[3] || vmax != geometry[4])
        return HMM_JPEG_OTHER_GEOMETRY;

    uint8_t* out = static_cast<uint8_t*>(slot);
    uint16_t* qt = reinterpret_cast<uint16_t*>(out);
    memset(out, 0, hmm::kJpegQtBytes);
    for (int c = 0; c < f.ncomp; ++c) memcpy(qt + 64 * c, f.q[f.tq[c]], 64 * sizeof(uint16_t));
    int16_t* blocks = reinterpret_cast<int16_t*>(out + hmm::kJpegQtBytes);

    const int mcux = f.ncomp == 1 ? hmm::jpeg_cdiv(f.W, 8) : hmm::jpeg_cdiv(f.W, 8 * hmax);
    const int mcuy = f.ncomp == 1 ? hmm::jpeg_cdiv(f.H, 8) : hmm::jpeg_cdiv(f.H, 8 * vmax);
    const int hs[3] = {hmax, 1, 1}, vs[3] = {vmax, 1, 1};
    Bits b{data, n, f.scan};
    int pred[3] = {0, 0, 0};
    int rst = 0;
    const int64_t total = (int64_t)mcux * mcuy;
    for (int64_t m = 0; m < total; ++m) {
        if (f.restart && m && m % f.restart == 0) {
            if (!b.marker_is(0xD0 + (rst & 7))) return HMM_JPEG_UNSUPPORTED;
            ++rst;
            pred[0] = pred[1] = pred[2] = 0;
        }
        const int mx = (int)(m % mcux), my = (int)(m / mcux);
        for (int c = 0; c < f.ncomp; ++c) {
            const Huff &dc = f.dc[f.td[c]], &ac = f.ac[f.ta[c]];
            const uint16_t* q = f.q[f.tq[c]];
            for (int v = 0; v < vs[c]; ++v)
                for (int u = 0; u < hs[c]; ++u) {
                    const int bx = mx * hs[c] + u - L.bx0[c], by = my * vs[c] + v - L.by0[c];
                    int16_t* dst = nullptr;
                    if (bx >= 0 && bx < L.nbx[c] && by >= 0 && by < L.nby[c])
                        dst = blocks + 64 * (L.block_off[c] + (int64_t)by * L.nbx[c] + bx);
                    if (!block(b, dc, ac, q, pred[c], dst)) return HMM_JPEG_UNSUPPORTED;
                }
        }
        if (b.nbits < b.npad) return HMM_JPEG_UNSUPPORTED;                 // read past the end of the data
    }
    if (!b.marker_is(0xD9)) return HMM_JPEG_UNSUPPORTED;                   // EOI right after the scan (no DNL, no second scan)
    return HMM_JPEG_DECODED;
}

// ---- the device entropy route: the host's share ---------------------------------------------------------------------------------
// Marker parse as above, then the scan's entropy bytes without their FF 00 stuffing plus the tables the kernel needs, into a
// bitstream slot (jpeg_entropy_core.h).  No Huffman decoding here: that is jpeg_entropy.hip's.  Files with a restart interval,
// with more than four distinct Huffman tables in use, or whose scan does not run up to an EOI marker keep the host entropy pass.

extern "C" int64_t hmm_jpeg_entropy_slot_bytes(size_t file_bytes) {
    return (int64_t)((file_bytes + (size_t)hmm::kEntropyDataOff + hmm::kEntropyPad + 255) / 256 * 256);
}

extern "C" int hmm_jpeg_prepare_entropy(const uint8_t* data, size_t n, const int32_t* geometry, void* slot, size_t slot_bytes) {
    HMM_REQUIRE(data && geometry && slot, HMM_E_INVALID, "jpeg_prepare_entropy: null pointer");
    HMM_REQUIRE(((uintptr_t)slot & 15) == 0, HMM_E_INVALID, "jpeg_prepare_entropy: the slot must be 16-byte aligned");
    Frame f;
    if (!parse(data, n, f)) return HMM_JPEG_UNSUPPORTED;
    const int hmax = f.ncomp == 3 ? f.hmax : 1, vmax = f.ncomp == 3 ? f.vmax : 1;
    if (f.W != geometry[0] || f.H != geometry[1] || f.ncomp != geometry[2] || hmax != geometry[3] || vmax != geometry[4])
        return HMM_JPEG_OTHER_GEOMETRY;
    if (f.restart) return HMM_JPEG_UNSUPPORTED;

    // The entropy segment: up to the first FF that is not followed by 00, which must be the EOI marker (marker_is(0xD9)).
    size_t stuffed = 0, end = 0;
    bool eoi = false;
    for (size_t i = f.scan; i < n;) {
        const uint8_t* p = static_cast<const uint8_t*>(memchr(data + i, 0xFF, n - i));
        if (!p) break;
        const size_t k = (size_t)(p - data);
        if (k + 1 < n && data[k + 1] == 0) {
            ++stuffed;
            i = k + 2;
            continue;
        }
        eoi = k + 1 < n && data[k + 1] == 0xD9;
        end = k;
        break;
    }
    if (!eoi) return HMM_JPEG_UNSUPPORTED;
    const size_t len = end - f.scan - stuffed;
    if (len > hmm::kEntropyMaxBytes) return HMM_JPEG_UNSUPPORTED;
    const size_t padded = (len + hmm::kEntropyPad - 1) / hmm::kEntropyPad * hmm::kEntropyPad;
    HMM_REQUIRE(slot_bytes >= (size_t)hmm::kEntropyDataOff + padded, HMM_E_WORKSPACE,
                "jpeg_prepare_entropy: slot of %zu bytes, %zu needed", slot_bytes, (size_t)hmm::kEntropyDataOff + padded);

    // Table slots: the distinct (class, id) pairs the components select, four at the most.
    int slot_class[4], slot_id[4], used = 0;
    uint32_t selectors = 0;
    for (int c = 0; c < f.ncomp; ++c)
        for (int ac = 0; ac < 2; ++ac) {
            const int id = ac ? f.ta[c] : f.td[c];
            int s = 0;
            while (s < used && !(slot_class[s] == ac && slot_id[s] == id)) ++s;
            if (s == used) {
                if (used == 4) return HMM_JPEG_UNSUPPORTED;
                slot_class[used] = ac;
                slot_id[used++] = id;
            }
            selectors |= (uint32_t)s << (4 * c + 2 * ac);
        }

    uint8_t* out = static_cast<uint8_t*>(slot);
    memset(out, 0, hmm::kEntropyDataOff);
    int32_t* head = reinterpret_cast<int32_t*>(out);
    head[hmm::kEhMagic] = (int32_t)hmm::kEntropyMagic;
    head[hmm::kEhBytes] = (int32_t)len;
    head[hmm::kEhComps] = f.ncomp;
    head[hmm::kEhHmax] = hmax;
    head[hmm::kEhVmax] = vmax;
    head[hmm::kEhSelectors] = (int32_t)selectors;
    head[hmm::kEhPadded] = (int32_t)padded;
    uint16_t* qt = reinterpret_cast<uint16_t*>(out + hmm::kEntropyQtOff);
    for (int c = 0; c < f.ncomp; ++c) memcpy(qt + 64 * c, f.q[f.tq[c]], 64 * sizeof(uint16_t));
    hmm::EntropyHuff* tables = reinterpret_cast<hmm::EntropyHuff*>(out + hmm::kEntropyHuffOff);
    for (int s = 0; s < used; ++s) {
        const Huff& h = slot_class[s] ? f.ac[slot_id[s]] : f.dc[slot_id[s]];
        hmm::EntropyHuff& t = tables[s];
        memcpy(t.look, h.look, sizeof(t.look));
        int count = 0;
        for (int l = 1; l <= 16; ++l) {
            t.maxcode[l] = h.maxcode[l];
            t.valoff[l] = h.bits[l] ? h.valoff[l] : 0;
            count += h.bits[l];
        }
        t.maxcode[0] = t.maxcode[17] = -1;
        memcpy(t.vals, h.vals, (size_t)count);
    }

    uint8_t* dst = out + hmm::kEntropyDataOff;
    for (size_t i = f.scan; i < end;) {
        const uint8_t* p = static_cast<const uint8_t*>(memchr(data + i, 0xFF, end - i));
        const size_t k = p ? (size_t)(p - data) + 1 : end;            // through the FF; its 00 is dropped
        memcpy(dst, data + i, k - i);
        dst += k - i;
        i = p ? k + 1 : end;
    }
    memset(dst, 0, padded - len);
    return HMM_JPEG_DECODED;
}
