// Host half of the baseline JPEG encoder: the bytes FF D8 .. SOS of a file as libjpeg writes them under Pillow's defaults
// (jcmarker.c), and the quantisation tables of a quality (jcparam.c).  No GPU call.
//
// Layout: SOI; APP0 "JFIF" 1.01, units 0, density 1 x 1, no thumbnail; one DQT segment per table (8-bit entries in zigzag
// order); SOF0; one DHT segment per table in the order DC 0, AC 0, DC 1, AC 1 (grey: the first two); SOS with Ss 0, Se 63, Ah/Al 0.
#include <string.h>

#include "hmm_common.h"
#include "jpeg_layout.h"

using namespace hmm;

namespace {

struct Out {
    uint8_t* p;
    size_t n = 0;
    void u8(int v) { p[n++] = (uint8_t)v; }
    void u16(int v) {
        u8(v >> 8);
        u8(v & 255);
    }
    void marker(int m, int payload) {
        u8(0xFF);
        u8(m);
        u16(payload + 2);
    }
};

// jpeg_set_quality(quality, force_baseline = TRUE): jpeg_quality_scaling, then (entry * scale + 50) / 100 limited to 1..255.
void quant_table(const uint8_t* base, int quality, uint16_t* out) {
    const int q = quality < 1 ? 1 : (quality > 100 ? 100 : quality);
    const int scale = q < 50 ? 5000 / q : 200 - 2 * q;
    for (int i = 0; i < 64; ++i) {
        const int v = (base[i] * scale + 50) / 100;
        out[i] = (uint16_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
    }
}

void dht(Out& o, int ident, const JpegStdHuff& t) {
    o.marker(0xC4, 1 + 16 + t.nvals);
    o.u8(ident);
    for (int i = 0; i < 16; ++i) o.u8(t.bits[i]);
    for (int i = 0; i < t.nvals; ++i) o.u8(t.vals[i]);
}

}  // namespace

extern "C" int hmm_jpeg_encode_header(const int32_t* geometry, int quality, uint8_t* header_out, size_t header_capacity,
                                      uint16_t* qtables_out) {
    HMM_REQUIRE(geometry && header_out && qtables_out, HMM_E_INVALID, "jpeg_encode_header: null pointer");
    JpegEncLayout L;
    HMM_REQUIRE(jpeg_enc_layout(geometry[0], geometry[1], geometry[2], geometry[3], geometry[4], &L), HMM_E_INVALID,
                "jpeg_encode_header: bad geometry (%d x %d, %d components, sampling %d x %d)", geometry[0], geometry[1], geometry[2],
                geometry[3], geometry[4]);
    HMM_REQUIRE(quality >= 1 && quality <= 100, HMM_E_INVALID, "jpeg_encode_header: quality %d outside 1..100", quality);
    HMM_REQUIRE(header_capacity >= L.header_bytes, HMM_E_INVALID, "jpeg_encode_header: room for %zu bytes, %u needed", header_capacity,
                L.header_bytes);
    quant_table(kJpegStdLumaQ, quality, qtables_out);
    quant_table(kJpegStdChromaQ, quality, qtables_out + 64);
    Out o{header_out};
    o.u8(0xFF);
    o.u8(0xD8);
    o.marker(0xE0, 14);
    for (const char* c = "JFIF"; *c; ++c) o.u8(*c);
    o.u8(0);
    o.u16(0x0101);
    o.u8(0);
    o.u16(1);
    o.u16(1);
    o.u16(0);
    for (int t = 0; t < (L.ncomp == 3 ? 2 : 1); ++t) {
        o.marker(0xDB, 65);
        o.u8(t);
        for (int k = 0; k < 64; ++k) o.u8(qtables_out[64 * t + kJpegZigzag[k]]);
    }
    o.marker(0xC0, 6 + 3 * L.ncomp);
    o.u8(8);
    o.u16(L.h);
    o.u16(L.w);
    o.u8(L.ncomp);
    for (int c = 0; c < L.ncomp; ++c) {
        o.u8(c + 1);
        o.u8(c == 0 ? (L.hs << 4 | L.vs) : 0x11);
        o.u8(c == 0 ? 0 : 1);
    }
    dht(o, 0x00, kJpegStdDcLuma);
    dht(o, 0x10, kJpegStdAcLuma);
    if (L.ncomp == 3) {
        dht(o, 0x01, kJpegStdDcChroma);
        dht(o, 0x11, kJpegStdAcChroma);
    }
    o.marker(0xDA, 4 + 2 * L.ncomp);
    o.u8(L.ncomp);
    for (int c = 0; c < L.ncomp; ++c) {
        o.u8(c + 1);
        o.u8(c == 0 ? 0x00 : 0x11);
    }
    o.u8(0);
    o.u8(63);
    o.u8(0);
    HMM_REQUIRE(o.n == L.header_bytes, HMM_E_INVALID, "jpeg_encode_header: wrote %zu bytes, %u expected", o.n, L.header_bytes);
    return (int)o.n;
}
