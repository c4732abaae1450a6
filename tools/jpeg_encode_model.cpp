// CPU model of the device JPEG encoder: the functions of hippomm_amd/csrc/jpeg_encode_core.h, run thread by thread with a loop
// where the kernels of jpeg_encode.hip have a barrier or a launch boundary.  Stand-alone: built together with
// hippomm_amd/csrc/jpeg_encode_host.cpp, no GPU call, so a sanitizer can watch every access the kernels' logic makes.  Every
// buffer is exactly as large as the library asks for and filled with a poison byte first.
//
//   jpeg_encode_model MANIFEST
//
// MANIFEST: one line per case, "pixels_path out_path W H channels bgr hs vs quality out_stride" (out_stride 0: the bound).  Reads
// the packed u8 pixels, writes the file (the slot's first `bytes` bytes) and prints one line per case with the status, the
// length and a census of what the scan contains.  Exit status 0 unless a file cannot be read or written.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../hippomm_amd/csrc/hmm_common.h"
#include "../hippomm_amd/csrc/jpeg_encode_core.h"

namespace hmm {
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputc('\n', stderr);
}
}  // namespace hmm

extern "C" int hmm_jpeg_encode_header(const int32_t* geometry, int quality, uint8_t* header_out, size_t header_capacity,
                                      uint16_t* qtables_out);

using namespace hmm;

static const JpegHuffEnc kHuff[4] = {jpeg_huff_enc(kJpegStdDcLuma), jpeg_huff_enc(kJpegStdAcLuma), jpeg_huff_enc(kJpegStdDcChroma),
                                     jpeg_huff_enc(kJpegStdAcChroma)};

struct HostWords {
    std::vector<uint32_t>& w;
    void or_word(uint32_t i, uint32_t v) { w.at(i) |= v; }
    void set_word(uint32_t i, uint32_t v) { w.at(i) = v; }
};

// Counts the codes that begin in one 32-bit word of the stream and end in the next.
struct StraddleCounter {
    uint32_t at, straddles = 0;
    void put(uint32_t, uint32_t len) {
        if (len && (at & 31) + len > 32) ++straddles;
        at += len;
    }
};

struct Census {
    int zrl = 0, max_zrl_block = 0, no_eob = 0, ac_cat_max = 0, stuffed = 0, last_ff = 0, straddle = 0;
    uint32_t dc_cats = 0;                        // bit k: a DC difference of category k occurs
};

static int table_of(const JpegEncLayout& L, uint32_t b) { return (L.ncomp == 3 && b % (uint32_t)L.bpm >= (uint32_t)(L.hs * L.vs)) ? 2 : 0; }

// What hmm_jpeg_encode does for one frame.  -> status; *bytes the length.
static int model_encode(const std::vector<uint8_t>& px, const JpegEncLayout& L, int channels, int bgr, const uint16_t* qt,
                        const std::vector<uint8_t>& header, std::vector<uint8_t>& out, uint64_t* bytes, Census* cs) {
    const uint8_t poison = 0xA5;
    std::vector<int16_t> coefs((size_t)L.blocks * 64, (int16_t)0xA5A5);
    std::vector<uint32_t> offs((size_t)L.blocks + 1, 0xA5A5A5A5u);
    std::vector<uint32_t> bits(L.bit_bytes / 4, 0xA5A5A5A5u);
    memset(out.data(), poison, out.size());
    std::fill(bits.begin(), bits.end(), 0u);                               // the call's memset

    // jpeg_fdct_kernel: 8 threads per block, a barrier between the passes
    for (uint32_t b = 0; b < L.blocks; ++b) {
        const EncBlock e = enc_block_at(L, b);
        int32_t ws[64], nat[64];
        for (int t = 0; t < 8; ++t) {
            int32_t d[8], o[8];
            enc_sample_row(px.data(), L, channels, bgr, e.comp, e.bx, e.by, t, d);
            enc_fdct_1d(d, o, true);
            for (int k = 0; k < 8; ++k) ws[t * 8 + k] = o[k];
        }
        const uint16_t* q = qt + (e.comp ? 64 : 0);
        for (int t = 0; t < 8; ++t) {
            int32_t d[8], o[8];
            for (int k = 0; k < 8; ++k) d[k] = ws[k * 8 + t];
            enc_fdct_1d(d, o, false);
            for (int k = 0; k < 8; ++k) nat[k * 8 + t] = (e.dummy && (k | t)) ? 0 : enc_quantise(o[k], q[k * 8 + t]);
        }
        for (int k = 0; k < 64; ++k) coefs[(size_t)b * 64 + k] = (int16_t)nat[kJpegZigzag[k]];
    }
    // jpeg_size_kernel: one thread sizes one block; jpeg_scan_kernel: the workgroup's prefix sum, here a running total
    uint32_t carry = 0;
    for (uint32_t b = 0; b < L.blocks; ++b) {
        const int64_t pb = enc_pred_block(L, b);
        const int32_t pred = pb < 0 ? 0 : coefs[(size_t)pb * 64];
        EncBitCounter counter;
        const int t = table_of(L, b);
        enc_block_bits(&coefs[(size_t)b * 64], pred, kHuff[t], kHuff[t + 1], counter);
        offs[b] = carry;
        carry += counter.bits;
        // census
        const int16_t* zz = &coefs[(size_t)b * 64];
        cs->dc_cats |= 1u << enc_category(zz[0] - pred);
        int run = 0, zrl = 0;
        for (int k = 1; k < 64; ++k) {
            if (!zz[k]) {
                ++run;
                continue;
            }
            zrl += run / 16;
            run = 0;
            if (enc_category(zz[k]) > cs->ac_cat_max) cs->ac_cat_max = enc_category(zz[k]);
        }
        cs->zrl += zrl;
        if (zrl > cs->max_zrl_block) cs->max_zrl_block = zrl;
        if (zz[63]) ++cs->no_eob;
        StraddleCounter sc{offs[b]};
        enc_block_bits(zz, pred, kHuff[t], kHuff[t + 1], sc);
        cs->straddle += sc.straddles;
    }
    offs[L.blocks] = carry;
    const uint32_t total = carry;
    const bool fits = ((uint64_t)total + 7) / 8 <= L.bit_bytes;
    // jpeg_emit_kernel: one thread per block, in an order that is not the scan's
    if (fits) {
        HostWords words{bits};
        for (uint32_t i = 0; i < L.blocks; ++i) {
            const uint32_t b = (i & 1) ? L.blocks - 1 - i / 2 : i / 2;   // 0, last, 1, last - 1, ...
            const int64_t pb = enc_pred_block(L, b);
            const int32_t pred = pb < 0 ? 0 : coefs[(size_t)pb * 64];
            const int t = table_of(L, b);
            EncBitWriter<HostWords> writer(words, offs[b]);
            enc_block_bits(&coefs[(size_t)b * 64], pred, kHuff[t], kHuff[t + 1], writer);
            if (b + 1 == L.blocks) {
                const uint32_t pad = (8 - (total & 7)) & 7;
                if (pad) writer.put((1u << pad) - 1, pad);
            }
            writer.finish();
        }
    }
    // jpeg_stuff_kernel: 16 bytes per thread and step; count, prefix sum, scatter
    const uint32_t used = fits ? (total + 7) / 8 : 0;
    const uint64_t limit = out.size();
    for (uint32_t i = 0; i < L.header_bytes && i < limit; ++i) out[i] = header[i];
    uint32_t ff = 0;
    for (uint32_t first = 0; first < used; first += kEncStuffBytes) {
        const uint32_t* w = &bits.at(first / 4);
        (void)bits.at(first / 4 + 3);                                      // the thread loads all four words
        const uint32_t mine = enc_count_ff(w, first, used);
        enc_scatter(w, first, used, ff, L.header_bytes, out.data(), limit);
        ff += mine;
    }
    cs->stuffed = (int)ff;
    cs->last_ff = used && enc_stream_byte(bits.data(), used - 1) == 0xFF;
    const uint64_t size = (uint64_t)L.header_bytes + used + ff + 2;
    *bytes = size;
    if (!fits || size > limit) return HMM_JPEG_ENCODE_OVERFLOW;
    out[size - 2] = 0xFF;
    out[size - 1] = 0xD9;
    for (uint64_t i = size; i < limit; ++i)
        if (out[i] != poison) return -100;                                 // wrote behind the file's end
    return HMM_JPEG_ENCODED;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s MANIFEST\n", argv[0]);
        return 2;
    }
    FILE* mf = fopen(argv[1], "r");
    if (!mf) return 2;
    char in_path[4096], out_path[4096];
    int W, H, channels, bgr, hs, vs, quality;
    long long stride;
    int cases = 0;
    while (fscanf(mf, "%4095s %4095s %d %d %d %d %d %d %d %lld", in_path, out_path, &W, &H, &channels, &bgr, &hs, &vs, &quality, &stride) == 10) {
        ++cases;
        const int32_t g[6] = {W, H, channels, hs, vs, 0};
        JpegEncLayout L;
        if (!jpeg_enc_layout(W, H, channels, hs, vs, &L)) return 3;
        std::vector<uint8_t> px((size_t)W * H * channels);
        FILE* f = fopen(in_path, "rb");
        if (!f || fread(px.data(), 1, px.size(), f) != px.size()) return 4;
        fclose(f);
        std::vector<uint8_t> header(L.header_bytes);
        uint16_t qt[128];
        if (hmm_jpeg_encode_header(g, quality, header.data(), header.size(), qt) != (int)L.header_bytes) return 5;
        const uint64_t bound = (uint64_t)L.header_bytes + 2 * (((uint64_t)L.blocks * kJpegMaxBlockBits + 7) / 8) + 2;
        std::vector<uint8_t> out(stride > 0 ? (size_t)stride : (size_t)bound);
        uint64_t bytes = 0;
        Census cs;
        const int status = model_encode(px, L, channels, bgr, qt, header, out, &bytes, &cs);
        if (status == HMM_JPEG_ENCODED) {
            f = fopen(out_path, "wb");
            if (!f || fwrite(out.data(), 1, (size_t)bytes, f) != (size_t)bytes) return 6;
            fclose(f);
        }
        printf("%s status=%d bytes=%llu blocks=%u zrl=%d max_zrl_block=%d no_eob=%d dc_cats=%u ac_cat_max=%d stuffed=%d last_ff=%d "
               "straddle=%d\n",
               out_path, status, (unsigned long long)bytes, L.blocks, cs.zrl, cs.max_zrl_block, cs.no_eob, cs.dc_cats, cs.ac_cat_max,
               cs.stuffed, cs.last_ff, cs.straddle);
    }
    fclose(mf);
    printf("cases=%d\n", cases);
    return 0;
}
