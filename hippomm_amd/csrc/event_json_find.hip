// hmm_json_find_matrices ON THE GPU: where the `[[numbers], ...]` matrices of an event file lie, from the text on the device, so that
// parse_event_features(matrices="device") no longer walks the file on the host before its kernels start.  The rules are stated in
// event_json_find_core.h; this file is the launch sequence around them and their host twin.
//
// The text is cut into groups of HMM_JSON_PARSE_GROUP_BYTES bytes, one workgroup of 256 threads each, 16 bytes per thread, staged in
// LDS as event_json_parse.hip stages them (one byte in front, HMM_JSON_TOKEN_MAX + 1 behind; bytes outside the text are spaces and
// are never dereferenced).  Eight launches on the caller's stream:
//   1. find_summary_kernel   per group: its string map, and for each of the three incoming string states the class and place of its
//                            last non-whitespace byte;
//   2. find_state_scan_kernel  one workgroup, 256 groups per round with a running carry: the string state, the class and the place
//                            in front of every group;
//   3. find_apply_kernel<COUNT>  per group, now with its incoming state: token starts, row starts, illegal bytes, long tokens,
//                            candidates and recorded events of the group;
//   4. find_count_scan_kernel  one workgroup: those counts as 64-bit exclusive prefixes;
//   5. find_apply_kernel<EMIT>  the same judgement again; every candidate, and every closer whose previous event is a candidate, goes
//                            into the event list with its prefix counts, in document order;
//   6. find_pair_kernel      one workgroup: each candidate against the entry behind it -> the matrices that only lack the row check;
//   7. find_apply_kernel<ROWS>  every row start inside such a matrix is checked against its place k * cols;
//   8. find_finish_kernel    one workgroup: the matrices that passed, in order, into out[0 .. min(n_found, cap)), and the report.
// No allocation, no synchronisation, no workgroup waits for another (the scans are single workgroups between launches), no scratch.
// All per-byte results are written with ordinary stores; the only atomics are 64-bit minima for the offset a decline names.
#include "hmm_common.h"
#include "event_json_find_core.h"

#include <vector>

namespace {

using namespace hmm;
namespace hf = hmm_find;

constexpr int kThreads = 256;
constexpr uint32_t kGroup = HMM_JSON_PARSE_GROUP_BYTES;
static_assert(kGroup == kThreads * hf::kBytesPerThread, "16 bytes of text per thread");
static_assert(HMM_JSON_PARSE_SCAN_GROUPS_PER_ROUND == kThreads, "the scans take one group per thread and round");
static_assert(sizeof(hmm_json_find_report) == 32 && sizeof(hmm_json_matrix) == 32, "the header's layouts");
static_assert(sizeof(hf::Event) == 48 && sizeof(hf::Matrix) == 64, "workspace entries");

constexpr uint64_t kMaxCands = HMM_JSON_FIND_MAX_CANDIDATES;
constexpr uint64_t kMaxEvents = 2 * kMaxCands;
constexpr uint64_t kNoOffset = HMM_JSON_PARSE_NO_OFFSET;

// ---- workspace, in 64-bit words ----
enum Header : int { kHdrRecorded = 0, kHdrCands = 1, kHdrOverflowAt = 2, kHdrDeclinedAt = 3, kHdrMatrices = 4, kHdrDeclined = 5, kHdrWords = 16 };
constexpr uint64_t kSummaryWords = 2, kIncomingWords = 2, kCountWords = 8;
enum Count : int { kCntTokens = 0, kCntRows = 1, kCntBad = 2, kCntLong = 3, kCntCands = 4, kCntRecorded = 5, kCntEventFlags = 6 };

struct Layout {
    uint64_t* header;
    uint64_t* summary;       // per group: variant 0 | variant 1 << 32, variant 2 | map << 32
    uint64_t* incoming;      // per group: string state | class << 8, place of the last non-whitespace byte
    uint64_t* counts;        // per group: kCountWords
    hf::Event* events;
    hf::Matrix* matrices;
};
inline uint64_t layout_words(uint64_t groups) {
    return kHdrWords + groups * (kSummaryWords + kIncomingWords + kCountWords) + kMaxEvents * (sizeof(hf::Event) / 8) +
           kMaxCands * (sizeof(hf::Matrix) / 8);
}
inline Layout layout_of(uint64_t* ws, uint64_t groups) {
    Layout l;
    l.header = ws;
    l.summary = l.header + kHdrWords;
    l.incoming = l.summary + groups * kSummaryWords;
    l.counts = l.incoming + groups * kIncomingWords;
    l.events = reinterpret_cast<hf::Event*>(l.counts + groups * kCountWords);
    l.matrices = reinterpret_cast<hf::Matrix*>(l.events + kMaxEvents);
    return l;
}

// events of a run of groups: {n recorded, flags} with n too large for events_compose's 13 bits
struct GroupEvents { uint32_t n, flags; };
HMM_JSON_HD GroupEvents group_events_compose(GroupEvents a, GroupEvents b) {
    if (!(b.flags & hf::kEvHas)) return a;
    if (!(a.flags & hf::kEvHas)) return b;
    GroupEvents r;
    r.n = a.n + b.n + (((b.flags & hf::kEvFirstCloser) && (a.flags & hf::kEvLastCand)) ? 1u : 0u);
    r.flags = hf::kEvHas | (a.flags & hf::kEvFirstCloser) | (b.flags & hf::kEvLastCand);
    return r;
}

// One thread's events into the list.  recorded: entries in front of the thread; last_cand: the event in front is a candidate; at0: the
// text offset of the thread's first byte; place_in: the place of the last non-whitespace byte in front of the thread; t, r, b, l: the
// prefix counts in front of the thread.  put(slot, event).
template <typename Put>
HMM_JSON_HD void emit_events(const hf::Walk& w, uint64_t recorded, bool last_cand, uint64_t at0, uint64_t place_in, uint64_t t, uint64_t r,
                             uint64_t b, uint64_t l, const Put& put) {
    uint32_t ev = w.cand | w.closer;
    while (ev) {
        const uint32_t bit = ev & (0u - ev), below = bit - 1;
        ev ^= bit;
        const bool is_cand = (w.cand & bit) != 0;
        if (is_cand || last_cand) {
            const uint32_t i = (uint32_t)__builtin_ctz(bit);
            hf::Event e;
            if (is_cand) {
                const uint32_t front = w.nonws & below;            // the first bracket: the last non-whitespace byte in front
                if (front) {
                    e.pos = at0 + (31 - (uint32_t)__builtin_clz(front));
                } else {
                    e.pos = place_in;
                }
            } else {
                e.pos = at0 + i + 1;
            }
            e.kind = is_cand ? hf::kEventCand : hf::kEventCloser;
            e.tokens = t + (uint64_t)__builtin_popcount(w.tok & below);
            e.rows = r + (uint64_t)__builtin_popcount(w.row & below);
            e.bad = b + (uint64_t)__builtin_popcount(w.bad & below);
            e.longs = l + (uint64_t)__builtin_popcount(w.lng & below);
            put(recorded++, e);
        }
        last_cand = is_cand;
    }
}

// the matrix of the list that holds text offset `at` behind its first bracket (which may itself look like a row start), or -1
HMM_JSON_HD int64_t matrix_at(const hf::Matrix* m, uint64_t n, uint64_t at) {
    uint64_t lo = 0, hi = n;                                      // the first entry with begin >= at
    while (lo < hi) {
        const uint64_t mid = (lo + hi) / 2;
        if (m[mid].begin >= at) hi = mid;
        else lo = mid + 1;
    }
    if (lo == 0) return -1;
    return at < m[lo - 1].end ? (int64_t)(lo - 1) : -1;
}

// ---- device ----
constexpr uint32_t kWindowBytes = 1 + kGroup + HMM_JSON_TOKEN_MAX + 1;
constexpr uint32_t kWindowVecs = (kWindowBytes + 15 + 15) / 16;

// Fill `vecs` with the 16-byte memory words that cover [one byte in front of the group at text offset `at`, the group,
// HMM_JSON_TOKEN_MAX + 1 bytes behind]; bytes outside text[0, n) become spaces and are not read.  Returns the LDS byte index of the
// group's first byte.  One barrier at the end.  (event_json_parse.hip stages its spans the same way.)
__device__ __forceinline__ uint32_t stage_window(const char* __restrict__ text, uint64_t n, uint64_t at, uint4* vecs) {
    const uintptr_t first = reinterpret_cast<uintptr_t>(text) + at - 1;
    const uintptr_t base = first & ~(uintptr_t)15;
    const uintptr_t lo = reinterpret_cast<uintptr_t>(text), hi = lo + n;
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
    return (uint32_t)(first - base) + 1;
}

struct LdsAt {
    const unsigned char* p;                                       // the thread's first byte
    __device__ __forceinline__ uint32_t operator()(int k) const { return p[k]; }
};

// Exclusive scan over the workgroup of N words per thread under an associative op(a, b, r) (a in front; r may alias neither):
// excl: what lies in front of the thread, total: the whole workgroup's.  lds: 4 * N words.  Two barriers.
template <int N, typename Op>
__device__ __forceinline__ void wg_scan(const uint32_t (&x)[N], const uint32_t (&ident)[N], const Op& op, uint32_t* lds, uint32_t (&excl)[N],
                                        uint32_t (&total)[N]) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl[N], y[N], r[N];
#pragma unroll
    for (int j = 0; j < N; ++j) incl[j] = x[j];
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
#pragma unroll
        for (int j = 0; j < N; ++j) y[j] = __shfl_up(incl[j], off, 64);
        op(y, incl, r);
        if (lane >= (uint32_t)off) {
#pragma unroll
            for (int j = 0; j < N; ++j) incl[j] = r[j];
        }
    }
    uint32_t prev[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        prev[j] = __shfl_up(incl[j], 1, 64);
        if (lane == 0) prev[j] = ident[j];
        if (lane == 63) lds[wave * N + j] = incl[j];
    }
    __syncthreads();
    uint32_t front[N], all[N];
#pragma unroll
    for (int j = 0; j < N; ++j) front[j] = all[j] = ident[j];
#pragma unroll
    for (uint32_t w = 0; w < kThreads / 64; ++w) {
        uint32_t s[N];
#pragma unroll
        for (int j = 0; j < N; ++j) s[j] = lds[w * N + j];
        op(all, s, r);
#pragma unroll
        for (int j = 0; j < N; ++j) all[j] = r[j];
        if (w < wave) {
#pragma unroll
            for (int j = 0; j < N; ++j) front[j] = all[j];
        }
    }
    op(front, prev, r);
#pragma unroll
    for (int j = 0; j < N; ++j) {
        excl[j] = r[j];
        total[j] = all[j];
    }
    __syncthreads();
}

template <int N>
struct AddOp {
    __device__ __forceinline__ void operator()(const uint32_t (&a)[N], const uint32_t (&b)[N], uint32_t (&r)[N]) const {
#pragma unroll
        for (int j = 0; j < N; ++j) r[j] = a[j] + b[j];
    }
};
struct MapOp {
    __device__ __forceinline__ void operator()(const uint32_t (&a)[1], const uint32_t (&b)[1], uint32_t (&r)[1]) const { r[0] = hf::map_compose(a[0], b[0]); }
};
struct LastOp {
    __device__ __forceinline__ void operator()(const uint32_t (&a)[1], const uint32_t (&b)[1], uint32_t (&r)[1]) const { r[0] = hf::last_compose(a[0], b[0]); }
};
struct EventsOp {
    __device__ __forceinline__ void operator()(const uint32_t (&a)[1], const uint32_t (&b)[1], uint32_t (&r)[1]) const { r[0] = hf::events_compose(a[0], b[0]); }
};
struct GroupEventsOp {
    __device__ __forceinline__ void operator()(const uint32_t (&a)[2], const uint32_t (&b)[2], uint32_t (&r)[2]) const {
        const GroupEvents g = group_events_compose(GroupEvents{a[0], a[1]}, GroupEvents{b[0], b[1]});
        r[0] = g.n;
        r[1] = g.flags;
    }
};
// {class, place low, place high} of the last non-whitespace byte of a run of groups; class kNone: no such byte
struct GroupLastOp {
    __device__ __forceinline__ void operator()(const uint32_t (&a)[3], const uint32_t (&b)[3], uint32_t (&r)[3]) const {
        const bool keep = b[0] == hf::kNone;
        r[0] = hf::last_class_behind(a[0], b[0]);
        r[1] = keep ? a[1] : b[1];
        r[2] = keep ? a[2] : b[2];
    }
};

// the string map of the bytes in front of the thread within its group, and the group's
__device__ __forceinline__ uint32_t map_in_front(const LdsAt& at, uint32_t count, uint32_t* lds, uint32_t* group_map) {
    uint32_t m[1] = {hf::kMapIdentity};
    for (uint32_t i = 0; i < hf::kBytesPerThread; ++i)
        if (i < count) m[0] = hf::map_compose(m[0], hf::byte_map(at((int)i)));
    const uint32_t ident[1] = {hf::kMapIdentity};
    uint32_t excl[1], total[1];
    wg_scan<1>(m, ident, MapOp(), lds, excl, total);
    *group_map = total[0];
    return excl[0];
}

// `last` of a walk with offsets counted from the group's first byte
__device__ __forceinline__ uint32_t last_in_group(uint32_t last) { return last ? last + hf::kBytesPerThread * threadIdx.x : 0u; }

__global__ __launch_bounds__(kThreads) void find_summary_kernel(const char* __restrict__ text, uint64_t len, uint64_t* __restrict__ summary) {
    __shared__ uint4 vecs[kWindowVecs];
    __shared__ uint32_t lds[16];
    const uint64_t at0 = (uint64_t)blockIdx.x * kGroup + hf::kBytesPerThread * threadIdx.x;
    const uint32_t lead = stage_window(text, len, (uint64_t)blockIdx.x * kGroup, vecs);
    const LdsAt at{reinterpret_cast<const unsigned char*>(vecs) + lead + hf::kBytesPerThread * threadIdx.x};
    const uint32_t count = hf::bytes_in_text(len, at0);
    uint32_t group_map;
    const uint32_t front_map = map_in_front(at, count, lds, &group_map);
    uint32_t variant[3];
#pragma unroll
    for (uint32_t s = 0; s < 3; ++s) {
        hf::Walk w;
        hf::walk(at, count, at0 == 0, hf::map_apply(front_map, s), hf::kNone, false, &w);
        const uint32_t x[1] = {last_in_group(w.last)}, ident[1] = {0};
        uint32_t excl[1], total[1];
        wg_scan<1>(x, ident, LastOp(), lds, excl, total);
        variant[s] = total[0];
    }
    if (threadIdx.x == 0) {
        summary[kSummaryWords * blockIdx.x] = (uint64_t)variant[0] | ((uint64_t)variant[1] << 32);
        summary[kSummaryWords * blockIdx.x + 1] = (uint64_t)variant[2] | ((uint64_t)group_map << 32);
    }
}

__global__ __launch_bounds__(kThreads) void find_state_scan_kernel(const uint64_t* __restrict__ summary, uint32_t groups, uint64_t* __restrict__ incoming) {
    __shared__ uint32_t lds[16];
    uint32_t state = hf::kOut, cls = hf::kQ;                      // in front of the text: nothing a matrix could continue
    uint64_t place = 0;
    for (uint32_t base = 0; base < groups; base += kThreads) {
        const uint32_t g = base + threadIdx.x;
        const bool live = g < groups;
        const uint64_t w0 = live ? summary[kSummaryWords * g] : 0, w1 = live ? summary[kSummaryWords * g + 1] : 0;
        const uint32_t m[1] = {live ? (uint32_t)(w1 >> 32) : hf::kMapIdentity}, ident_map[1] = {hf::kMapIdentity};
        uint32_t front_map[1], all_map[1];
        wg_scan<1>(m, ident_map, MapOp(), lds, front_map, all_map);
        const uint32_t state_in = hf::map_apply(front_map[0], state);
        const uint32_t v = state_in == 0 ? (uint32_t)w0 : state_in == 1 ? (uint32_t)(w0 >> 32) : (uint32_t)w1;
        const uint64_t at = (uint64_t)g * kGroup + (v & 0xFFFF);
        const uint32_t x[3] = {live ? v >> 16 : (uint32_t)hf::kNone, (uint32_t)at, (uint32_t)(at >> 32)}, ident[3] = {hf::kNone, 0, 0};
        uint32_t front[3], all[3];
        wg_scan<3>(x, ident, GroupLastOp(), lds, front, all);
        if (live) {
            const bool keep = front[0] == hf::kNone;
            incoming[kIncomingWords * g] = state_in | (hf::last_class_behind(cls, front[0]) << 8);
            incoming[kIncomingWords * g + 1] = keep ? place : ((uint64_t)front[2] << 32) | front[1];
        }
        state = hf::map_apply(all_map[0], state);
        if (all[0] != hf::kNone) place = ((uint64_t)all[2] << 32) | all[1];
        cls = hf::last_class_behind(cls, all[0]);
    }
}

enum Mode : int { kModeCount = 0, kModeEmit = 1, kModeRows = 2 };

template <int MODE>
__global__ __launch_bounds__(kThreads) void find_apply_kernel(const char* __restrict__ text, uint64_t len, Layout l) {
    __shared__ uint4 vecs[kWindowVecs];
    __shared__ uint32_t lds[16];
    if (MODE == kModeRows && (l.header[kHdrMatrices] == 0 || l.header[kHdrDeclined] != 0)) return;
    const uint32_t g = blockIdx.x;
    const uint64_t at0 = (uint64_t)g * kGroup + hf::kBytesPerThread * threadIdx.x;
    const uint32_t lead = stage_window(text, len, (uint64_t)g * kGroup, vecs);
    const LdsAt at{reinterpret_cast<const unsigned char*>(vecs) + lead + hf::kBytesPerThread * threadIdx.x};
    const uint32_t count = hf::bytes_in_text(len, at0);
    const uint64_t in0 = l.incoming[kIncomingWords * g], place_g = l.incoming[kIncomingWords * g + 1];
    uint32_t group_map;
    const uint32_t state = hf::map_apply(map_in_front(at, count, lds, &group_map), (uint32_t)(in0 & 0xFF));
    hf::Walk w;
    hf::walk(at, count, at0 == 0, state, hf::kNone, false, &w);
    uint32_t front_last[1], all_last[1];
    {
        const uint32_t x[1] = {last_in_group(w.last)}, ident[1] = {0};
        wg_scan<1>(x, ident, LastOp(), lds, front_last, all_last);
    }
    const uint32_t cls_in = hf::last_class_behind((uint32_t)(in0 >> 8), front_last[0] >> 16);
    const uint64_t place_in = (front_last[0] >> 16) == hf::kNone ? place_g : (uint64_t)g * kGroup + (front_last[0] & 0xFFFF);
    hf::walk(at, count, at0 == 0, state, cls_in, MODE != kModeRows, &w);

    const uint32_t sums[2] = {(uint32_t)__popc(w.tok) | ((uint32_t)__popc(w.row) << 16), (uint32_t)__popc(w.bad) | ((uint32_t)__popc(w.lng) << 16)};
    const uint32_t zero2[2] = {0, 0};
    uint32_t front[2], all[2];
    wg_scan<2>(sums, zero2, AddOp<2>(), lds, front, all);
    uint64_t* cnt = l.counts + kCountWords * g;
    if (MODE == kModeRows) {
        const uint64_t tokens = cnt[kCntTokens] + (front[0] & 0xFFFF), rows = cnt[kCntRows] + (front[0] >> 16);
        const uint64_t n = l.header[kHdrMatrices];
        uint32_t left = w.row;
        while (left) {
            const uint32_t bit = left & (0u - left), below = bit - 1;
            left ^= bit;
            const int64_t j = matrix_at(l.matrices, n, at0 + (uint32_t)__popc(below));
            if (j >= 0 && !hf::row_in_place(l.matrices[j], rows + (uint32_t)__popc(w.row & below), tokens + (uint32_t)__popc(w.tok & below)))
                l.matrices[j].ragged = 1;
        }
        return;
    }
    const uint32_t ev[1] = {hf::events_of(w.cand, w.closer)}, zero1[1] = {0};
    uint32_t front_ev[1], all_ev[1];
    wg_scan<1>(ev, zero1, EventsOp(), lds, front_ev, all_ev);
    if (MODE == kModeCount) {
        if (threadIdx.x == 0) {
            cnt[kCntTokens] = all[0] & 0xFFFF;
            cnt[kCntRows] = all[0] >> 16;
            cnt[kCntBad] = all[1] & 0xFFFF;
            cnt[kCntLong] = all[1] >> 16;
            cnt[kCntCands] = all_ev[0] >> hf::kEvCandShift;
            cnt[kCntRecorded] = all_ev[0] & hf::kEvCountMask;
            cnt[kCntEventFlags] = all_ev[0] & (hf::kEvHas | hf::kEvFirstCloser | hf::kEvLastCand);
        }
        return;
    }
    if (!(w.cand | w.closer)) return;
    const bool group_last_cand = cnt[kCntEventFlags] != 0;
    const bool has = (front_ev[0] & hf::kEvHas) != 0;
    const uint64_t recorded = cnt[kCntRecorded] + (front_ev[0] & hf::kEvCountMask) + ((has && (front_ev[0] & hf::kEvFirstCloser) && group_last_cand) ? 1 : 0);
    const bool last_cand = has ? (front_ev[0] & hf::kEvLastCand) != 0 : group_last_cand;
    hf::Event* events = l.events;
    uint64_t* header = l.header;
    emit_events(w, recorded, last_cand, at0, place_in, cnt[kCntTokens] + (front[0] & 0xFFFF), cnt[kCntRows] + (front[0] >> 16),
                cnt[kCntBad] + (front[1] & 0xFFFF), cnt[kCntLong] + (front[1] >> 16), [=](uint64_t slot, const hf::Event& e) {
                    if (slot < kMaxEvents) events[slot] = e;
                    else atomicMin(reinterpret_cast<unsigned long long*>(header + kHdrOverflowAt), (unsigned long long)e.pos);
                });
}

// The per-group counts -> exclusive prefixes in place (kCntRecorded: list entries in front of the group; kCntEventFlags: is the event
// in front of the group a candidate), the totals into the header, which is opened here.
__global__ __launch_bounds__(kThreads) void find_count_scan_kernel(uint64_t* __restrict__ counts, uint32_t groups, uint64_t* __restrict__ header) {
    __shared__ uint32_t lds[32];
    uint64_t carry[5] = {0, 0, 0, 0, 0}, carry_n = 0;
    bool carry_last_cand = false;
    for (uint32_t base = 0; base < groups; base += kThreads) {
        const uint32_t g = base + threadIdx.x;
        const bool live = g < groups;
        uint64_t* cnt = counts + kCountWords * g;
        uint32_t x[5];
#pragma unroll
        for (int j = 0; j < 5; ++j) x[j] = live ? (uint32_t)cnt[j] : 0u;
        const uint32_t e[2] = {live ? (uint32_t)cnt[kCntRecorded] : 0u, live ? (uint32_t)cnt[kCntEventFlags] : 0u};
        const uint32_t zero5[5] = {0, 0, 0, 0, 0}, zero2[2] = {0, 0};
        uint32_t front[5], all[5], front_ev[2], all_ev[2];
        wg_scan<5>(x, zero5, AddOp<5>(), lds, front, all);
        wg_scan<2>(e, zero2, GroupEventsOp(), lds, front_ev, all_ev);
        if (live) {
#pragma unroll
            for (int j = 0; j < 5; ++j) cnt[j] = carry[j] + front[j];
            const bool has = (front_ev[1] & hf::kEvHas) != 0;
            cnt[kCntRecorded] = carry_n + (has ? front_ev[0] + (((front_ev[1] & hf::kEvFirstCloser) && carry_last_cand) ? 1 : 0) : 0);
            cnt[kCntEventFlags] = has ? ((front_ev[1] & hf::kEvLastCand) ? 1 : 0) : (carry_last_cand ? 1 : 0);
        }
#pragma unroll
        for (int j = 0; j < 5; ++j) carry[j] += all[j];
        if (all_ev[1] & hf::kEvHas) {
            carry_n += all_ev[0] + (((all_ev[1] & hf::kEvFirstCloser) && carry_last_cand) ? 1 : 0);
            carry_last_cand = (all_ev[1] & hf::kEvLastCand) != 0;
        }
    }
    if (threadIdx.x == 0) {
        header[kHdrRecorded] = carry_n;
        header[kHdrCands] = carry[kCntCands];
        header[kHdrOverflowAt] = kNoOffset;
        header[kHdrDeclinedAt] = kNoOffset;
        header[kHdrMatrices] = 0;
        header[kHdrDeclined] = 0;
    }
}

__global__ __launch_bounds__(kThreads) void find_pair_kernel(Layout l, uint64_t min_values) {
    __shared__ uint32_t lds[4];
    const uint64_t n = l.header[kHdrRecorded];
    if (n > kMaxEvents) {                                          // uniform
        if (threadIdx.x == 0) {
            l.header[kHdrDeclined] = 1;
            l.header[kHdrDeclinedAt] = l.header[kHdrOverflowAt];
        }
        return;
    }
    uint64_t found = 0;
    for (uint64_t base = 0; base + 1 < n; base += kThreads) {
        const uint64_t i = base + threadIdx.x;
        hf::Matrix m;
        int r = hf::kNoMatrix;
        if (i + 1 < n) r = hf::pair_events(l.events[i], l.events[i + 1], min_values, &m);
        if (r == hf::kDeclineLong) {
            atomicMin(reinterpret_cast<unsigned long long*>(l.header + kHdrDeclinedAt), (unsigned long long)l.events[i].pos);
            l.header[kHdrDeclined] = 1;
        }
        const uint32_t x[1] = {r == hf::kMatrix ? 1u : 0u}, zero[1] = {0};
        uint32_t front[1], all[1];
        wg_scan<1>(x, zero, AddOp<1>(), lds, front, all);
        if (r == hf::kMatrix) l.matrices[found + front[0]] = m;
        found += all[0];
    }
    if (threadIdx.x == 0) l.header[kHdrMatrices] = found;
}

__global__ __launch_bounds__(kThreads) void find_finish_kernel(Layout l, hmm_json_matrix* __restrict__ out, uint64_t cap,
                                                               hmm_json_find_report* __restrict__ report) {
    __shared__ uint32_t lds[4];
    const bool declined = l.header[kHdrDeclined] != 0;
    const uint64_t n = declined ? 0 : l.header[kHdrMatrices];
    uint64_t found = 0;
    for (uint64_t base = 0; base < n; base += kThreads) {
        const uint64_t i = base + threadIdx.x;
        const bool good = i < n && l.matrices[i].ragged == 0;
        const uint32_t x[1] = {good ? 1u : 0u}, zero[1] = {0};
        uint32_t front[1], all[1];
        wg_scan<1>(x, zero, AddOp<1>(), lds, front, all);
        const uint64_t slot = found + front[0];
        if (good && slot < cap) {
            const hf::Matrix m = l.matrices[i];
            out[slot] = hmm_json_matrix{(size_t)m.begin, (size_t)m.end, (size_t)m.rows, (size_t)m.cols};
        }
        found += all[0];
    }
    if (threadIdx.x == 0) {
        report->n_found = found;
        report->n_candidates = l.header[kHdrCands];
        report->status = declined ? HMM_JSON_FIND_DECLINED : HMM_JSON_FIND_OK;
        report->first_declined = declined ? l.header[kHdrDeclinedAt] : kNoOffset;
    }
}

// ---- the host twin: the same pieces, the scans as plain loops in thread order ----
struct HostAt {
    const unsigned char* text;
    uint64_t len, at0;
    uint32_t operator()(int k) const {
        const uint64_t p = at0 + (uint64_t)(int64_t)k;            // k == -1 in front of the text wraps behind its end
        return p < len ? text[p] : (uint32_t)' ';
    }
};

struct HostGroup {
    hf::Walk w[kThreads];
    uint64_t place_in[kThreads];
};

// one group with its incoming state, as find_apply_kernel sees it
void host_apply(const unsigned char* text, uint64_t len, uint64_t g, uint32_t state_g, uint32_t cls_g, uint64_t place_g, bool judge, HostGroup* out) {
    uint32_t state = state_g, last = 0;
    for (uint32_t t = 0; t < (uint32_t)kThreads; ++t) {
        const uint64_t at0 = g * kGroup + hf::kBytesPerThread * t;
        const HostAt at{text, len, at0};
        const uint32_t count = hf::bytes_in_text(len, at0);
        hf::Walk first;
        hf::walk(at, count, at0 == 0, state, hf::kNone, false, &first);
        const uint32_t cls_in = hf::last_class_behind(cls_g, last >> 16);
        out->place_in[t] = (last >> 16) == hf::kNone ? place_g : g * kGroup + (last & 0xFFFF);
        hf::walk(at, count, at0 == 0, state, cls_in, judge, &out->w[t]);
        last = hf::last_compose(last, first.last ? first.last + hf::kBytesPerThread * t : 0u);
        state = hf::map_apply(first.map, state);
    }
}

}  // namespace

extern "C" size_t hmm_json_find_matrices_device_workspace_bytes(size_t len) {
    if (len < 1 || len > HMM_JSON_PARSE_MAX_SPAN_BYTES) return 0;
    return layout_words((len + kGroup - 1) / kGroup) * sizeof(uint64_t);
}

extern "C" int hmm_json_find_matrices_device(const char* text_dev, size_t len, size_t min_values, hmm_json_matrix* out_dev, int cap,
                                             hmm_json_find_report* report_dev, void* workspace_dev, size_t workspace_bytes, hmm_stream_t stream) {
    HMM_REQUIRE(text_dev && report_dev && workspace_dev && (out_dev || cap == 0), HMM_E_INVALID, "json_find_matrices_device: null pointer");
    HMM_REQUIRE(cap >= 0, HMM_E_INVALID, "json_find_matrices_device: cap %d is negative", cap);
    HMM_REQUIRE(len >= 1 && len <= HMM_JSON_PARSE_MAX_SPAN_BYTES, HMM_E_INVALID, "json_find_matrices_device: a text of %zu bytes, 1 to %llu in one call",
                len, (unsigned long long)HMM_JSON_PARSE_MAX_SPAN_BYTES);
    HMM_REQUIRE(workspace_bytes >= hmm_json_find_matrices_device_workspace_bytes(len), HMM_E_INVALID,
                "json_find_matrices_device: workspace of %zu bytes, need %zu", workspace_bytes, hmm_json_find_matrices_device_workspace_bytes(len));
    HMM_REQUIRE(reinterpret_cast<uintptr_t>(out_dev) % 8 == 0 && reinterpret_cast<uintptr_t>(workspace_dev) % 8 == 0 &&
                    reinterpret_cast<uintptr_t>(report_dev) % 8 == 0,
                HMM_E_INVALID, "json_find_matrices_device: out, report and workspace must be aligned to 8 bytes");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint32_t groups = (uint32_t)((len + kGroup - 1) / kGroup);
    const Layout l = layout_of(static_cast<uint64_t*>(workspace_dev), groups);
    find_summary_kernel<<<groups, kThreads, 0, st>>>(text_dev, len, l.summary);
    HMM_LAUNCH_CHECK();
    find_state_scan_kernel<<<1, kThreads, 0, st>>>(l.summary, groups, l.incoming);
    HMM_LAUNCH_CHECK();
    find_apply_kernel<kModeCount><<<groups, kThreads, 0, st>>>(text_dev, len, l);
    HMM_LAUNCH_CHECK();
    find_count_scan_kernel<<<1, kThreads, 0, st>>>(l.counts, groups, l.header);
    HMM_LAUNCH_CHECK();
    find_apply_kernel<kModeEmit><<<groups, kThreads, 0, st>>>(text_dev, len, l);
    HMM_LAUNCH_CHECK();
    find_pair_kernel<<<1, kThreads, 0, st>>>(l, (uint64_t)min_values);
    HMM_LAUNCH_CHECK();
    find_apply_kernel<kModeRows><<<groups, kThreads, 0, st>>>(text_dev, len, l);
    HMM_LAUNCH_CHECK();
    find_finish_kernel<<<1, kThreads, 0, st>>>(l, out_dev, (uint64_t)cap, report_dev);
    HMM_LAUNCH_CHECK();
    return HMM_OK;
}

extern "C" int hmm_json_find_matrices_blocks(const char* text_c, size_t len, size_t min_values, hmm_json_matrix* out, int cap,
                                             hmm_json_find_report* report) {
    HMM_REQUIRE(text_c && report && (out || cap == 0), HMM_E_INVALID, "json_find_matrices_blocks: null pointer");
    HMM_REQUIRE(cap >= 0, HMM_E_INVALID, "json_find_matrices_blocks: cap %d is negative", cap);
    HMM_REQUIRE(len >= 1 && len <= HMM_JSON_PARSE_MAX_SPAN_BYTES, HMM_E_INVALID, "json_find_matrices_blocks: a text of %zu bytes, 1 to %llu in one call",
                len, (unsigned long long)HMM_JSON_PARSE_MAX_SPAN_BYTES);
    const unsigned char* text = reinterpret_cast<const unsigned char*>(text_c);
    const uint64_t groups = (len + kGroup - 1) / kGroup;
    // 1. + 2. the summaries of every group under the three incoming string states, folded in group order
    struct Incoming { uint32_t state, cls; uint64_t place; };
    std::vector<Incoming> incoming(groups);
    {
        uint32_t state = hf::kOut, cls = hf::kQ;
        uint64_t place = 0;
        for (uint64_t g = 0; g < groups; ++g) {
            incoming[g] = Incoming{state, cls, place};
            uint32_t variant[3] = {0, 0, 0}, map = hf::kMapIdentity;
            for (uint32_t t = 0; t < (uint32_t)kThreads; ++t) {
                const uint64_t at0 = g * kGroup + hf::kBytesPerThread * t;
                const HostAt at{text, len, at0};
                const uint32_t count = hf::bytes_in_text(len, at0);
                hf::Walk w;
                for (uint32_t s = 0; s < 3; ++s) {
                    hf::walk(at, count, at0 == 0, hf::map_apply(map, s), hf::kNone, false, &w);
                    variant[s] = hf::last_compose(variant[s], w.last ? w.last + hf::kBytesPerThread * t : 0u);
                }
                map = hf::map_compose(map, w.map);
            }
            const uint32_t v = variant[state];
            if ((v >> 16) != hf::kNone) place = g * kGroup + (v & 0xFFFF);
            cls = hf::last_class_behind(cls, v >> 16);
            state = hf::map_apply(map, state);
        }
    }
    // 3. + 4. + 5. counts and events; the prefix counts run along
    std::vector<hf::Event> events;
    uint64_t tokens = 0, rows = 0, bad = 0, longs = 0, cands = 0, recorded = 0, overflow_at = kNoOffset;
    bool last_cand = false;
    std::vector<HostGroup> one(1);
    HostGroup& hg = one[0];
    for (uint64_t g = 0; g < groups; ++g) {
        host_apply(text, len, g, incoming[g].state, incoming[g].cls, incoming[g].place, true, &hg);
        // the group's events as the kernels count them: composed thread by thread, then placed behind the groups in front
        uint32_t ev = 0;
        uint64_t t_in = tokens, r_in = rows, b_in = bad, l_in = longs;
        for (uint32_t t = 0; t < (uint32_t)kThreads; ++t) {
            const hf::Walk& w = hg.w[t];
            const bool has = (ev & hf::kEvHas) != 0;
            const uint64_t slot = recorded + (ev & hf::kEvCountMask) + ((has && (ev & hf::kEvFirstCloser) && last_cand) ? 1 : 0);
            const bool lc = has ? (ev & hf::kEvLastCand) != 0 : last_cand;
            emit_events(w, slot, lc, g * kGroup + hf::kBytesPerThread * t, hg.place_in[t], t_in, r_in, b_in, l_in, [&](uint64_t at, const hf::Event& e) {
                if (at < kMaxEvents) {
                    if (events.size() <= at) events.resize(at + 1);
                    events[at] = e;
                } else if (e.pos < overflow_at) {
                    overflow_at = e.pos;
                }
            });
            ev = hf::events_compose(ev, hf::events_of(w.cand, w.closer));
            t_in += __builtin_popcount(w.tok); r_in += __builtin_popcount(w.row); b_in += __builtin_popcount(w.bad); l_in += __builtin_popcount(w.lng);
        }
        tokens = t_in; rows = r_in; bad = b_in; longs = l_in;
        cands += ev >> hf::kEvCandShift;
        if (ev & hf::kEvHas) {
            recorded += (ev & hf::kEvCountMask) + (((ev & hf::kEvFirstCloser) && last_cand) ? 1 : 0);
            last_cand = (ev & hf::kEvLastCand) != 0;
        }
    }
    report->n_candidates = cands;
    report->n_found = 0;
    report->status = HMM_JSON_FIND_OK;
    report->first_declined = kNoOffset;
    if (recorded > kMaxEvents) {
        report->status = HMM_JSON_FIND_DECLINED;
        report->first_declined = overflow_at;
        return HMM_OK;
    }
    // 6. pairs
    std::vector<hf::Matrix> matrices;
    uint64_t declined_at = kNoOffset;
    for (uint64_t i = 0; i + 1 < recorded && i + 1 < events.size(); ++i) {
        hf::Matrix m;
        const int r = hf::pair_events(events[i], events[i + 1], min_values, &m);
        if (r == hf::kDeclineLong && events[i].pos < declined_at) declined_at = events[i].pos;
        if (r == hf::kMatrix) matrices.push_back(m);
    }
    if (declined_at != kNoOffset) {
        report->status = HMM_JSON_FIND_DECLINED;
        report->first_declined = declined_at;
        return HMM_OK;
    }
    // 7. rows in place
    if (!matrices.empty()) {
        tokens = rows = 0;
        for (uint64_t g = 0; g < groups; ++g) {
            host_apply(text, len, g, incoming[g].state, incoming[g].cls, incoming[g].place, false, &hg);
            for (uint32_t t = 0; t < (uint32_t)kThreads; ++t) {
                const hf::Walk& w = hg.w[t];
                uint32_t left = w.row;
                while (left) {
                    const uint32_t bit = left & (0u - left), below = bit - 1;
                    left ^= bit;
                    const int64_t j = matrix_at(matrices.data(), matrices.size(), g * kGroup + hf::kBytesPerThread * t + (uint32_t)__builtin_popcount(below));
                    if (j >= 0 && !hf::row_in_place(matrices[j], rows + (uint32_t)__builtin_popcount(w.row & below), tokens + (uint32_t)__builtin_popcount(w.tok & below)))
                        matrices[j].ragged = 1;
                }
                tokens += __builtin_popcount(w.tok);
                rows += __builtin_popcount(w.row);
            }
        }
    }
    // 8. the list
    uint64_t found = 0;
    for (const hf::Matrix& m : matrices) {
        if (m.ragged) continue;
        if (found < (uint64_t)cap) out[found] = hmm_json_matrix{(size_t)m.begin, (size_t)m.end, (size_t)m.rows, (size_t)m.cols};
        ++found;
    }
    report->n_found = found;
    return HMM_OK;
}
