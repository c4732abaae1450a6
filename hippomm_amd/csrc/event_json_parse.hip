// The feature matrices of an event file read back ON THE GPU: the text of one `[[numbers], ...]` span, as hmm_json_find_matrices
// (event_json.cpp) reported it, becomes rows x cols fp32 or fp64 on the device -- for fp32 the bits hmm_json_parse_matrix_f32 gives,
// for fp64 the bits of np.array(json.loads(span)) -- without the text becoming Python floats or a host matrix.  The counterpart of
// event_json.hip, and the same shape: a prefix sum away from independent work.
//
// Inside a span there are no strings, so a byte is a SEPARATOR (space \n \r \t , [ ]), a NUMBER BYTE (digits + - . e E and the
// letters of NaN and Infinity) or wrong; a token starts at a number byte behind a separator, and its ordinal among the starts is
// its index in the matrix.  The span is cut into groups of HMM_JSON_PARSE_GROUP_BYTES bytes, counted from its first byte:
//   1. json_count_kernel:   one workgroup per group counts the token starts among its bytes into the workspace;
//   2. json_starts_scan_kernel: one workgroup turns the counts into 64-bit exclusive prefixes, HMM_JSON_PARSE_SCAN_GROUPS_PER_ROUND
//                           per round with a running carry, and opens the report: the token count, and whether it is rows x cols;
//   3. json_convert_kernel: the same workgroups find their starts again, scan them inside the workgroup, list the starts in LDS by
//                           ordinal -- so that conversion runs on dense lanes, not on the one lane in eight whose bytes hold a start --
//                           and convert token k with event_json_parse_core.h into out[k].
// A workgroup stages its bytes in LDS once: the 16-byte words that cover one byte in front of the group, the group and
// HMM_JSON_TOKEN_MAX + 1 bytes behind it (a token may run past the group's end), loaded as aligned uint4 wherever the word lies
// inside the span and byte by byte, guarded, at the span's two ends -- any begin, end and base alignment is correct and no byte
// outside [begin, end) is dereferenced.  Bytes outside the span count as spaces.  Every thread then classifies its 16 bytes from
// five dwords of LDS (lanes 16 bytes apart: 4 lanes per bank row, a 4-way conflict on 5 reads per thread; the token bytes are
// read as single bytes at scattered addresses).  Three launches on the caller's stream, no allocation, no synchronisation, no
// scratch, no workgroup waits for another.  The powers of ten are read from global memory (a __device__ array, 10 KB, L1/L2).
//
// Not checked here: the brackets and commas between the numbers.  The span finder is the authority on the structure of the file;
// this reads the numbers of a span it reported.
#include "hmm_common.h"
#include "event_json_parse_core.h"

namespace {

using namespace hmm;

constexpr int kThreads = 256;
constexpr int kBytesPerThread = 16;
constexpr uint32_t kGroup = HMM_JSON_PARSE_GROUP_BYTES;
static_assert(kGroup == kThreads * kBytesPerThread, "one uint4 of text per thread");
static_assert(HMM_JSON_PARSE_SCAN_GROUPS_PER_ROUND == kThreads, "the scan takes one count per thread and round");
static_assert(HMM_JSON_TOKEN_MAX >= 64 && HMM_JSON_TOKEN_MAX + 1 < (int)kGroup, "a token's tail is staged behind its group");
static_assert(sizeof(hmm_json_parse_report) == 32 && sizeof(hmm_json_flagged) == 32, "the header's layouts");
static_assert(HMM_JSON_FLAG_UNDECIDED == hmm_json::kUndecided && HMM_JSON_FLAG_RANGE == hmm_json::kOutOfRange &&
                  HMM_JSON_FLAG_TOO_LONG == hmm_json::kTooLong && HMM_JSON_FLAG_BAD_TOKEN == hmm_json::kBadToken,
              "the header names the core's flags");

// window: [one byte in front of the group, the group, HMM_JSON_TOKEN_MAX + 1 bytes behind], widened to whole 16-byte words of memory
constexpr uint32_t kWindowBytes = 1 + kGroup + HMM_JSON_TOKEN_MAX + 1;
constexpr uint32_t kWindowVecs = (kWindowBytes + 15 + 15) / 16;
constexpr uint32_t kMaxStarts = kGroup / 2;                    // "1,1,1,": every other byte

const uint64_t h_pow10[HMM_JSON_POW10_COUNT][2] = {HMM_JSON_POW10_ENTRIES};
__device__ uint64_t d_pow10[HMM_JSON_POW10_COUNT][2] = {HMM_JSON_POW10_ENTRIES};

// bit c of the pair: is the ASCII byte c a separator / a number byte
constexpr uint64_t bit_of(int c) { return 1ull << (c & 63); }
constexpr uint64_t kSepLo = bit_of(' ') | bit_of('\n') | bit_of('\r') | bit_of('\t') | bit_of(',');
constexpr uint64_t kSepHi = bit_of('[') | bit_of(']');
constexpr uint64_t kNumLo = bit_of('0') | bit_of('1') | bit_of('2') | bit_of('3') | bit_of('4') | bit_of('5') | bit_of('6') | bit_of('7') |
                            bit_of('8') | bit_of('9') | bit_of('+') | bit_of('-') | bit_of('.');
constexpr uint64_t kNumHi = bit_of('e') | bit_of('E') | bit_of('N') | bit_of('a') | bit_of('I') | bit_of('n') | bit_of('f') | bit_of('i') |
                            bit_of('t') | bit_of('y');
static_assert(' ' < 64 && ',' < 64 && '9' < 64 && '[' >= 64 && 'y' < 128, "ASCII");

__device__ __forceinline__ bool in_set(uint32_t c, uint64_t lo, uint64_t hi) {
    return c < 128 && (((c < 64 ? lo : hi) >> (c & 63)) & 1);
}
__device__ __forceinline__ bool is_separator(uint32_t c) { return in_set(c, kSepLo, kSepHi); }
__device__ __forceinline__ bool is_number_byte(uint32_t c) { return in_set(c, kNumLo, kNumHi); }

// Where a workgroup's window lies in LDS.
struct Window {
    uint32_t lead;       // LDS byte index of the byte in front of the group's first byte
};

// Fill `vecs` (kWindowVecs uint4 of LDS) with the memory words that cover the window of the group at span offset `at`; bytes outside
// span[0, n) become spaces.  One barrier at the end.
__device__ __forceinline__ Window stage_window(const char* __restrict__ span, uint64_t n, uint64_t at, uint4* vecs) {
    const uintptr_t first = reinterpret_cast<uintptr_t>(span) + at - 1;          // address of the byte in front of the group
    const uintptr_t base = first & ~(uintptr_t)15;
    const uintptr_t lo = reinterpret_cast<uintptr_t>(span), hi = lo + n;         // the span's addresses
    for (uint32_t v = threadIdx.x; v < kWindowVecs; v += kThreads) {
        const uintptr_t a = base + 16 * (uintptr_t)v;
        uint4 word;
        if (a >= lo && a + 16 <= hi) {
            word = *reinterpret_cast<const uint4*>(a);
        } else {
            uint32_t w[4];
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                uint32_t x = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const uintptr_t p = a + 4 * d + b;
                    const uint32_t c = (p >= lo && p < hi) ? (uint32_t)*reinterpret_cast<const unsigned char*>(p) : (uint32_t)' ';
                    x |= c << (8 * b);
                }
                w[d] = x;
            }
            word = make_uint4(w[0], w[1], w[2], w[3]);
        }
        vecs[v] = word;
    }
    __syncthreads();
    Window win;
    win.lead = (uint32_t)(first - base);
    return win;
}

// The thread's 16 bytes of the group (byte i of the thread is group byte 16 tid + i): bit i of *starts for a token start, bit i of
// *wrong for a byte that is neither a separator nor a number byte.  Bytes behind the span's end are spaces and give neither.
__device__ __forceinline__ void classify(const uint4* vecs, const Window& win, uint32_t* starts, uint32_t* wrong) {
    const uint32_t* words = reinterpret_cast<const uint32_t*>(vecs);
    const uint32_t at = win.lead + kBytesPerThread * threadIdx.x;               // LDS byte index of the byte in front of the thread's first
    const uint32_t s = 8 * (at & 3);                                             // the same for every thread
    uint32_t w[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) w[j] = words[(at >> 2) + j];
    // 17 bytes from bit s of w[0] on, as five aligned dwords
    uint32_t a[5];
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] = (uint32_t)(((((uint64_t)w[j + 1]) << 32) | w[j]) >> s);
    a[4] = w[4] >> s;
    uint32_t st = 0, bad = 0;
    bool prev_sep = is_separator(a[0] & 0xFF);
#pragma unroll
    for (int i = 0; i < kBytesPerThread; ++i) {
        const uint32_t c = (a[(i + 1) >> 2] >> (8 * ((i + 1) & 3))) & 0xFF;
        const bool sep = is_separator(c), num = is_number_byte(c);
        st |= (uint32_t)(num && prev_sep) << i;
        bad |= (uint32_t)(!sep && !num) << i;
        prev_sep = sep;
    }
    *starts = st;
    *wrong = bad;
}

// Inclusive scan over the 64 lanes, then over the workgroup's 4 waves through `sums` (kThreads / 64 words of LDS): the exclusive
// prefix of `x` within the workgroup, and the workgroup's total.  One barrier inside; `sums` may be written again after the caller's
// next one.  (event_json.hip has the same routine for its item lengths.)
__device__ __forceinline__ uint32_t group_exclusive_scan(uint32_t x, uint32_t* sums, uint32_t* total) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = x;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t up = __shfl_up(incl, off, 64);
        if (lane >= (uint32_t)off) incl += up;
    }
    if (lane == 63) sums[wave] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < kThreads / 64; ++w) {
        const uint32_t s = sums[w];
        before += w < wave ? s : 0;
        all += s;
    }
    *total = all;
    return before + incl - x;
}

__global__ __launch_bounds__(kThreads) void json_count_kernel(const char* __restrict__ span, uint64_t n, uint64_t* __restrict__ group_counts) {
    __shared__ uint4 vecs[kWindowVecs];
    __shared__ uint32_t sums[kThreads / 64];
    const Window win = stage_window(span, n, (uint64_t)blockIdx.x * kGroup, vecs);
    uint32_t starts, wrong;
    classify(vecs, win, &starts, &wrong);
    uint32_t count = __popc(starts);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) count += __shfl_xor(count, off, 64);
    if ((threadIdx.x & 63) == 0) sums[threadIdx.x >> 6] = count;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t all = 0;
        for (int w = 0; w < kThreads / 64; ++w) all += sums[w];
        group_counts[blockIdx.x] = all;
    }
}

// group_counts[0 .. n_groups) -> their exclusive prefix sums in place; the report is opened with the total.  One workgroup.
__global__ __launch_bounds__(kThreads) void json_starts_scan_kernel(uint64_t* __restrict__ group_counts, uint32_t n_groups, uint64_t expected,
                                                                    hmm_json_parse_report* __restrict__ report) {
    __shared__ uint64_t wave_sums[kThreads / 64];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t carry = 0;
    for (uint32_t base = 0; base < n_groups; base += HMM_JSON_PARSE_SCAN_GROUPS_PER_ROUND) {
        const uint32_t i = base + threadIdx.x;
        const uint64_t x = i < n_groups ? group_counts[i] : 0;
        uint64_t incl = x;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t lo = __shfl_up((uint32_t)incl, off, 64), hi = __shfl_up((uint32_t)(incl >> 32), off, 64);
            if (lane >= (uint32_t)off) incl += ((uint64_t)hi << 32) | lo;
        }
        if (lane == 63) wave_sums[wave] = incl;
        __syncthreads();
        uint64_t before = 0, all = 0;
#pragma unroll
        for (uint32_t w = 0; w < kThreads / 64; ++w) {
            const uint64_t s = wave_sums[w];
            before += w < wave ? s : 0;
            all += s;
        }
        if (i < n_groups) group_counts[i] = carry + before + incl - x;
        carry += all;
        __syncthreads();                                             // wave_sums is written again in the next round
    }
    if (threadIdx.x == 0) {
        report->n_tokens = carry;
        report->n_flagged = 0;
        report->first_bad = HMM_JSON_PARSE_NO_OFFSET;
        report->status = carry == expected ? HMM_JSON_PARSE_OK : HMM_JSON_PARSE_COUNT;
    }
}

// The report's words are only ever raised (status, n_flagged) or lowered (first_bad) by the convert kernel: order does not matter.
__device__ __forceinline__ void report_wrong(hmm_json_parse_report* report, uint64_t offset, uint64_t status) {
    atomicMin(reinterpret_cast<unsigned long long*>(&report->first_bad), (unsigned long long)offset);
    atomicMax(reinterpret_cast<unsigned long long*>(&report->status), (unsigned long long)status);
}

template <typename T>
__global__ __launch_bounds__(kThreads) void json_convert_kernel(const char* __restrict__ span, uint64_t n, uint64_t span_begin,
                                                                const uint64_t* __restrict__ group_firsts, uint64_t expected, T* __restrict__ out,
                                                                hmm_json_parse_report* __restrict__ report, hmm_json_flagged* __restrict__ flagged,
                                                                uint64_t flagged_cap) {
    __shared__ uint4 vecs[kWindowVecs];
    __shared__ uint32_t sums[kThreads / 64];
    __shared__ uint16_t start_at[kMaxStarts];                        // group byte offset of the workgroup's token starts, by ordinal
    const uint64_t at = (uint64_t)blockIdx.x * kGroup;
    const Window win = stage_window(span, n, at, vecs);
    uint32_t starts, wrong;
    classify(vecs, win, &starts, &wrong);
    if (wrong) report_wrong(report, span_begin + at + kBytesPerThread * threadIdx.x + (uint32_t)__ffs(wrong) - 1, HMM_JSON_PARSE_BAD_BYTE);
    uint32_t total;
    uint32_t ordinal = group_exclusive_scan(__popc(starts), sums, &total);
    while (starts) {
        const uint32_t i = (uint32_t)__ffs(starts) - 1;
        starts &= starts - 1;
        start_at[ordinal++] = (uint16_t)(kBytesPerThread * threadIdx.x + i);
    }
    __syncthreads();
    const unsigned char* bytes = reinterpret_cast<const unsigned char*>(vecs) + win.lead + 1;      // bytes[x]: group byte x
    const uint64_t first = group_firsts[blockIdx.x];
    for (uint32_t t = threadIdx.x; t < total; t += kThreads) {
        const uint32_t off = start_at[t];
        const uint64_t k = first + t;
        // the token's end: the first byte that is no number byte; the window holds HMM_JSON_TOKEN_MAX + 1 bytes behind every start
        int len = 1;
        while (len <= HMM_JSON_TOKEN_MAX && is_number_byte(bytes[off + len])) ++len;
        uint64_t bits = 0;
        int flag;
        uint64_t token_end = at + off + len;                         // span offsets
        if (len > HMM_JSON_TOKEN_MAX) {
            flag = hmm_json::kTooLong;
            while (token_end < n && is_number_byte((unsigned char)span[token_end])) ++token_end;
        } else {
            flag = hmm_json::parse_number(bytes + off, len, d_pow10, &bits);
        }
        if (flag == hmm_json::kBadToken) {
            report_wrong(report, span_begin + at + off, HMM_JSON_PARSE_BAD_TOKEN);
        } else if (flag != hmm_json::kParsed) {
            const uint64_t slot = atomicAdd(reinterpret_cast<unsigned long long*>(&report->n_flagged), 1ull);
            if (slot < flagged_cap) {
                hmm_json_flagged f;
                f.ordinal = k;
                f.begin = span_begin + at + off;
                f.end = span_begin + token_end;
                f.flag = (uint64_t)flag;
                flagged[slot] = f;
            }
        }
        if (k < expected) {                                          // more tokens than rows x cols: nothing is written behind the matrix
            if constexpr (sizeof(T) == 8) out[k] = bits;
            else out[k] = hmm_json::narrow_double_bits(bits);
        }
    }
}

template <typename T>
int launch_all(const char* span, uint64_t n, uint64_t span_begin, uint64_t expected, T* out, hmm_json_parse_report* report,
               hmm_json_flagged* flagged, uint64_t flagged_cap, uint64_t* ws, hipStream_t st) {
    const uint32_t groups = (uint32_t)((n + kGroup - 1) / kGroup);
    json_count_kernel<<<groups, kThreads, 0, st>>>(span, n, ws);
    HMM_LAUNCH_CHECK();
    json_starts_scan_kernel<<<1, kThreads, 0, st>>>(ws, groups, expected, report);
    HMM_LAUNCH_CHECK();
    json_convert_kernel<T><<<groups, kThreads, 0, st>>>(span, n, span_begin, ws, expected, out, report, flagged, flagged_cap);
    HMM_LAUNCH_CHECK();
    return HMM_OK;
}

}  // namespace

extern "C" size_t hmm_json_parse_matrix_device_workspace_bytes(size_t span_bytes) {
    if (span_bytes < 1 || span_bytes > HMM_JSON_PARSE_MAX_SPAN_BYTES) return 0;
    return (span_bytes + kGroup - 1) / kGroup * sizeof(uint64_t);
}

extern "C" int hmm_json_parse_matrix_device(const char* text_dev, size_t begin, size_t end, size_t rows, size_t cols, int dtype, void* out_dev,
                                            hmm_json_parse_report* report_dev, hmm_json_flagged* flagged_dev, int64_t flagged_cap,
                                            void* workspace_dev, size_t workspace_bytes, hmm_stream_t stream) {
    HMM_REQUIRE(text_dev && out_dev && report_dev && workspace_dev && (flagged_dev || flagged_cap == 0), HMM_E_INVALID,
                "json_parse_matrix_device: null pointer");
    HMM_REQUIRE(begin < end, HMM_E_INVALID, "json_parse_matrix_device: empty span [%zu, %zu)", begin, end);
    HMM_REQUIRE(end - begin <= HMM_JSON_PARSE_MAX_SPAN_BYTES, HMM_E_INVALID, "json_parse_matrix_device: a span of %zu bytes, at most %llu in one call",
                end - begin, (unsigned long long)HMM_JSON_PARSE_MAX_SPAN_BYTES);
    HMM_REQUIRE(dtype == HMM_JSON_DTYPE_F32 || dtype == HMM_JSON_DTYPE_F64, HMM_E_INVALID,
                "json_parse_matrix_device: dtype must be %d (fp32) or %d (fp64), got %d", HMM_JSON_DTYPE_F32, HMM_JSON_DTYPE_F64, dtype);
    HMM_REQUIRE(rows >= 1 && cols >= 1, HMM_E_INVALID, "json_parse_matrix_device: %zu x %zu values (at least 1 x 1)", rows, cols);
    HMM_REQUIRE(rows <= HMM_JSON_MAX_VALUES / cols, HMM_E_INVALID, "json_parse_matrix_device: %zu x %zu values, at most %llu are read in one call",
                rows, cols, (unsigned long long)HMM_JSON_MAX_VALUES);
    HMM_REQUIRE(flagged_cap >= 0, HMM_E_INVALID, "json_parse_matrix_device: flagged_cap %lld is negative", (long long)flagged_cap);
    HMM_REQUIRE(workspace_bytes >= hmm_json_parse_matrix_device_workspace_bytes(end - begin), HMM_E_INVALID,
                "json_parse_matrix_device: workspace of %zu bytes, need %zu", workspace_bytes,
                hmm_json_parse_matrix_device_workspace_bytes(end - begin));
    const size_t elem = dtype == HMM_JSON_DTYPE_F64 ? 8 : 4;
    HMM_REQUIRE(reinterpret_cast<uintptr_t>(out_dev) % elem == 0 && reinterpret_cast<uintptr_t>(workspace_dev) % 8 == 0 &&
                    reinterpret_cast<uintptr_t>(report_dev) % 8 == 0 && reinterpret_cast<uintptr_t>(flagged_dev) % 8 == 0,
                HMM_E_INVALID, "json_parse_matrix_device: out must be aligned to its element, report, flagged list and workspace to 8 bytes");
    hipStream_t st = static_cast<hipStream_t>(stream);
    uint64_t* ws = static_cast<uint64_t*>(workspace_dev);
    const uint64_t expected = (uint64_t)rows * cols;
    if (dtype == HMM_JSON_DTYPE_F64)
        return launch_all(text_dev + begin, end - begin, begin, expected, static_cast<uint64_t*>(out_dev), report_dev, flagged_dev,
                          (uint64_t)flagged_cap, ws, st);
    return launch_all(text_dev + begin, end - begin, begin, expected, static_cast<uint32_t*>(out_dev), report_dev, flagged_dev,
                      (uint64_t)flagged_cap, ws, st);
}

// The core of event_json_parse_core.h on the host: token i is text[spans[2 i], spans[2 i + 1]).
extern "C" int hmm_json_float_parse(const char* text, const uint64_t* spans, size_t n, uint64_t* out_f64_bits, uint32_t* out_f32_bits,
                                    int* out_flags) {
    HMM_REQUIRE((text && spans && out_f64_bits && out_f32_bits && out_flags) || n == 0, HMM_E_INVALID, "json_float_parse: null pointer");
    for (size_t i = 0; i < n; ++i) {
        const uint64_t b = spans[2 * i], e = spans[2 * i + 1];
        HMM_REQUIRE(b < e, HMM_E_INVALID, "json_float_parse: token %zu is empty", i);
        uint64_t bits = 0;
        out_flags[i] = e - b > HMM_JSON_TOKEN_MAX ? (int)hmm_json::kTooLong : hmm_json::parse_number(text + b, (int)(e - b), h_pow10, &bits);
        out_f64_bits[i] = bits;
        out_f32_bits[i] = hmm_json::narrow_double_bits(bits);
    }
    return HMM_OK;
}
