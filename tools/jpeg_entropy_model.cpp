// CPU model of the device entropy pass: the functions of hippomm_amd/csrc/jpeg_entropy_core.h, run thread by thread with a loop
// where the kernel has a barrier, against the host entropy pass (hmm_jpeg_decode_coefs) on the same files.  Stand-alone: built
// together with hippomm_amd/csrc/jpeg_host.cpp, no GPU call, so a sanitizer can watch every access the kernel's logic makes.
//
//   jpeg_entropy_model MANIFEST
//
// MANIFEST: one line per case, "path W H components hmax vmax x0 y0 w h".  Prints one line per case and exits 0 when, for
// every file the prepare pass takes, the model's status equals the host's and, where both decoded, the slots are equal bytes --
// with 256 threads per frame as on the device and with 3, where every thread owns several subsequences.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../hippomm_amd/csrc/hmm_common.h"
#include "../hippomm_amd/csrc/jpeg_entropy_core.h"

namespace hmm {
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputc('\n', stderr);
}
}  // namespace hmm

extern "C" int64_t hmm_jpeg_slot_bytes(const int32_t* geometry, int x0, int y0, int w, int h);
extern "C" int hmm_jpeg_decode_coefs(const uint8_t* data, size_t n, const int32_t* geometry, int x0, int y0, int w, int h, void* slot,
                                     size_t slot_bytes);
extern "C" int64_t hmm_jpeg_entropy_slot_bytes(size_t file_bytes);
extern "C" int hmm_jpeg_prepare_entropy(const uint8_t* data, size_t n, const int32_t* geometry, void* slot, size_t slot_bytes);

using namespace hmm;

// What jpeg_entropy_kernel and jpeg_entropy_finish_kernel do for one frame, with `threads` threads.  Every buffer is exactly as
// large as the library asks for and filled with `poison` first.
static int model_decode(const uint8_t* bs, size_t bitslot_bytes, const int32_t* g, const int win[4], uint8_t* slot, uint32_t threads,
                        uint8_t poison, uint32_t* rounds_out) {
    JpegLayout L;
    if (!jpeg_layout(g[0], g[1], g[2], g[3], g[4], win[0], win[1], win[2], win[3], &L)) return -1;
    const int hmax = g[2] == 3 ? g[3] : 1, vmax = g[2] == 3 ? g[4] : 1;
    const uint32_t total_blocks = entropy_total_blocks(g[0], g[1], g[2], g[3], g[4]);
    const EntropyWorkspace ws = entropy_workspace(total_blocks, bitslot_bytes);
    std::vector<uint64_t> wsmem(ws.frame_bytes / 8);
    uint8_t* wsf = reinterpret_cast<uint8_t*>(wsmem.data());
    memset(wsf, poison, ws.frame_bytes);
    memset(wsf, 0, ws.coef_bytes);                                          // the launch zeroes the coefficients
    memset(slot, poison, (size_t)L.slot_bytes);

    const int32_t* head = reinterpret_cast<const int32_t*>(bs);
    memcpy(slot, bs + kEntropyQtOff, kJpegQtBytes);
    const int64_t tail = kJpegQtBytes + L.block_off[L.ncomp] * kJpegBlockBytes;
    memset(slot + tail, 0, (size_t)(L.slot_bytes - tail));
    const uint32_t nbytes = (uint32_t)head[kEhBytes];
    const bool header_ok = (uint32_t)head[kEhMagic] == kEntropyMagic && head[kEhComps] == L.ncomp && head[kEhHmax] == hmax &&
                           head[kEhVmax] == vmax && nbytes <= kEntropyMaxBytes &&
                           (size_t)kEntropyDataOff + ((size_t)nbytes + 3) / 4 * 4 <= bitslot_bytes &&
                           entropy_subsequences(nbytes * 8) <= ws.max_sub;
    *rounds_out = 0;
    if (!header_ok) return HMM_JPEG_UNSUPPORTED;

    EntropyCtx c;
    c.words = reinterpret_cast<const uint32_t*>(bs + kEntropyDataOff);
    c.nwords = (nbytes + 3) / 4;
    c.total_bits = nbytes * 8;
    c.huff = reinterpret_cast<const EntropyHuff*>(bs + kEntropyHuffOff);
    c.selectors = (uint32_t)head[kEhSelectors];
    c.ncomp = L.ncomp;
    c.hv = L.ncomp == 3 ? hmax * vmax : 1;
    c.bpm = L.ncomp == 3 ? c.hv + 2 : 1;
    c.total_blocks = total_blocks;
    c.nsub = entropy_subsequences(c.total_bits);
    c.per = (c.nsub + threads - 1) / threads;
    c.entry = reinterpret_cast<uint64_t*>(wsf + ws.entry_off);
    c.count = reinterpret_cast<uint32_t*>(wsf + ws.count_off);
    c.dirty = reinterpret_cast<uint32_t*>(wsf + ws.dirty_off);
    c.coef = reinterpret_cast<int16_t*>(wsf);

    std::vector<uint64_t> boundary(threads);
    for (uint32_t t = 0; t < threads; ++t) entropy_init(c, t, boundary.data());
    uint32_t rounds = 0;
    bool converged = false;
    while (rounds <= c.nsub) {
        ++rounds;
        for (uint32_t t = 0; t < threads; ++t) entropy_round(c, t, boundary.data());
        bool changed = false;
        for (uint32_t t = 0; t < threads; ++t) changed |= entropy_sync(c, t, boundary.data());
        if (!changed) {
            converged = true;
            break;
        }
    }
    *rounds_out = rounds;

    std::vector<uint32_t> blocks(threads);
    std::vector<ThreadOut> th(threads);
    for (uint32_t t = 0; t < threads; ++t) blocks[t] = entropy_thread_blocks(c, t);
    uint32_t base = 0, end_bit = kNoEnd, bad = 0;
    for (uint32_t t = 0; t < threads; ++t) {
        entropy_write(c, t, base, th[t]);
        base += blocks[t];
        if (th[t].end_bit != kNoEnd) end_bit = th[t].end_bit;
        bad |= th[t].bad;
    }
    uint32_t r0 = 0, r1 = 0, r2 = 0;
    for (uint32_t t = 0; t < threads; ++t) {
        bad |= entropy_dc_walk(c, th[t], (int32_t)r0, (int32_t)r1, (int32_t)r2);
        r0 += th[t].d0;
        r1 += th[t].d1;
        r2 += th[t].d2;
    }
    if (!converged || bad || !entropy_end_ok(end_bit, c.total_bits)) return HMM_JPEG_UNSUPPORTED;

    bool refused = false;
    const int mcux = jpeg_cdiv(g[0], 8 * hmax);
    for (uint32_t b = 0; b < total_blocks; ++b)
        refused |= finish_block(c.coef, reinterpret_cast<const uint16_t*>(bs + kEntropyQtOff), L, mcux, c.hv, c.bpm, b, slot);
    return refused ? HMM_JPEG_UNSUPPORTED : HMM_JPEG_DECODED;
}

static bool read_file(const char* path, std::vector<uint8_t>& out) {
    FILE* fh = fopen(path, "rb");
    if (!fh) return false;
    fseek(fh, 0, SEEK_END);
    const long n = ftell(fh);
    fseek(fh, 0, SEEK_SET);
    out.resize(n > 0 ? (size_t)n : 0);
    const size_t got = out.empty() ? 0 : fread(out.data(), 1, out.size(), fh);
    fclose(fh);
    return got == out.size();
}

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s MANIFEST\n", argv[0]);
        return 2;
    }
    FILE* mf = fopen(argv[1], "r");
    if (!mf) {
        fprintf(stderr, "cannot open %s\n", argv[1]);
        return 2;
    }
    char path[4096];
    int32_t g[HMM_JPEG_GEOMETRY_INTS] = {0, 0, 0, 0, 0, 0};
    int win[4];
    int failures = 0, cases = 0, taken = 0, decoded = 0;
    while (fscanf(mf, "%4095s %d %d %d %d %d %d %d %d %d", path, &g[0], &g[1], &g[2], &g[3], &g[4], &win[0], &win[1], &win[2], &win[3]) == 10) {
        ++cases;
        std::vector<uint8_t> data;
        if (!read_file(path, data)) {
            printf("%s unreadable\n", path);
            ++failures;
            continue;
        }
        if (data.empty()) data.reserve(1);
        const size_t bsb = (size_t)hmm_jpeg_entropy_slot_bytes(data.size());
        std::vector<uint64_t> bsmem(bsb / 8 + 2);                                       // 16-byte aligned, exactly bsb bytes used
        uint8_t* bs = reinterpret_cast<uint8_t*>(bsmem.data());
        bs += (16 - ((uintptr_t)bs & 15)) & 15;
        const uint8_t* bytes = data.empty() ? reinterpret_cast<const uint8_t*>("") : data.data();
        const int prep = hmm_jpeg_prepare_entropy(bytes, data.size(), g, bs, bsb);
        const int64_t sb = hmm_jpeg_slot_bytes(g, win[0], win[1], win[2], win[3]);
        if (sb <= 0) {
            printf("%s bad window\n", path);
            ++failures;
            continue;
        }
        std::vector<uint8_t> host_slot((size_t)sb, 0);
        const int host = hmm_jpeg_decode_coefs(bytes, data.size(), g, win[0], win[1], win[2], win[3], host_slot.data(), host_slot.size());
        if (prep != HMM_JPEG_DECODED) {
            // the prepare pass refuses nothing the host pass would decode, apart from restart intervals and table counts
            printf("%s prepare=%d host=%d\n", path, prep, host);
            if (prep < 0 || prep > HMM_JPEG_OTHER_GEOMETRY) ++failures;
            continue;
        }
        ++taken;
        const uint32_t thread_counts[2] = {(uint32_t)kEntropyThreads, 3};
        const uint8_t poisons[2] = {0xFF, 0x7F};
        for (int k = 0; k < 2; ++k) {
            std::vector<uint8_t> slot((size_t)sb);
            uint32_t rounds = 0;
            const int st = model_decode(bs, bsb, g, win, slot.data(), thread_counts[k], poisons[k], &rounds);
            const bool same = st == host && (st != HMM_JPEG_DECODED || memcmp(slot.data(), host_slot.data(), (size_t)sb) == 0);
            printf("%s threads=%u prepare=%d host=%d model=%d rounds=%u %s\n", path, thread_counts[k], prep, host, st, rounds,
                   same ? "ok" : "MISMATCH");
            if (!same) ++failures;
            if (k == 0 && st == HMM_JPEG_DECODED) ++decoded;
        }
    }
    fclose(mf);
    printf("cases=%d taken=%d decoded=%d failures=%d\n", cases, taken, decoded, failures);
    return failures ? 1 : 0;
}
