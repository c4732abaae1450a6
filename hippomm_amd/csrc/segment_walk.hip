// The window walk of _segment_sequence (hippomm/core/hippocampal_memory.py:1002-1114) on gfx950 with its control loop on the device:
// "where does the segment that starts here end?", step after step, over resident inputs -- the SSIM score of every adjacent frame
// pair (hmm_ssim_pairs), the frame times, the audio track -- so that a video needs one read-back, of the segment list.
//
// The loop is ordered: a step starts where the previous one ended.  The order is the stream's, nothing waits for another workgroup.
//   video only   one launch, one thread walks every step: a step is two binary searches over the times and a scan of a window's
//                pairs from the end, a few dozen fp64 loads.
//   with audio   a step needs the sums of squares of its 500 ms windows first, and those are window_sums_kernel's (audio_track.hip,
//                numpy's summation order) -- a kernel of one workgroup per window that reads its (start, length) table from device
//                memory.  So: one planning launch writes the table of step 0; then per step one launch of that kernel over
//                max_windows table rows and one decide launch, which takes the step and writes the table of the next one.  Rows
//                past the step's windows, and every row once the walk has ended, have length 0: such a workgroup reads nothing.
//                A track of int16 samples (hmm_segment_walk_pcm16) takes pcm16_window_sums_kernel there instead: fp64 sums, exact,
//                the bits the fp64 track of x / 32768.0 gives, so everything behind the sums is the fp64 walk unchanged.
// The arithmetic on times is fp64, operation by operation the reference's Python floats (contraction is off in this file).  The level
// of a window never becomes dB here: the caller passes rms_cut, the least rms whose level under the caller's own log10 is not below
// the silence threshold, and the comparison is made on the rms.  Frame indices come from device memory (times_dev) by binary
// search and lie in [0, n_frames) by construction; n_segments is checked against max_steps before it indexes the records.
#include "audio_levels.h"

#include <cmath>

#pragma clang fp contract(off)

namespace hmm {

constexpr int kWalkThreads = 256;

struct WalkArgs {
    const double* scores;
    const int32_t* flags;
    const double* times;
    int n_frames;
    int has_audio, track_f64;
    int64_t track_len, sample_rate, window;
    double total, max_dur, min_dur, sim_threshold, rms_cut;
    int silent_without_rms, max_windows, max_steps;
};

// What a step that starts at `start` looks at: its end, and its audio windows lo_k = S + first_off - k * window, k < n_windows.
struct StepSpan {
    double end;
    int64_t S, first_off;
    int64_t n_windows;
};

__device__ __forceinline__ double py_min(double a, double b) { return b < a ? b : a; }      // Python's min(a, b)

__device__ __forceinline__ StepSpan step_span(const WalkArgs& a, double start) {
    StepSpan sp;
    sp.end = py_min(start + a.max_dur, a.total);
    sp.S = 0;
    sp.first_off = 0;
    sp.n_windows = 0;
    if (a.has_audio) {
        const double sr = (double)a.sample_rate;
        sp.S = (int64_t)(start * sr);                                        // int(current_start * audio_sample_rate)
        const int64_t E = (int64_t)(sp.end * sr);
        sp.first_off = E - sp.S - a.window;                                  // range(E - S - window, 0, -window)
        if (sp.first_off > 0) sp.n_windows = (sp.first_off + a.window - 1) / a.window;
    }
    return sp;
}

// Row k of the table: window k of the span clipped to the track as audio_data[lo:lo + window] clips, or (0, 0) past the span's windows.
__device__ __forceinline__ void write_table(const WalkArgs& a, const StepSpan& sp, bool running, int64_t* __restrict__ table) {
    for (int k = threadIdx.x; k < a.max_windows; k += kWalkThreads) {
        int64_t lo = 0, len = 0;
        if (running && k < sp.n_windows) {
            const int64_t at = sp.S + sp.first_off - (int64_t)k * a.window;
            lo = at < a.track_len ? at : a.track_len;
            len = (at + a.window < a.track_len ? at + a.window : a.track_len) - lo;
        }
        table[2 * k] = lo;
        table[2 * k + 1] = len;
    }
}

// The first index in [0, n] whose time is not below x (strict == false) or above x (strict == true).
__device__ __forceinline__ int time_bound(const double* __restrict__ times, int n, double x, bool strict) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        const double t = times[mid];
        if (strict ? t <= x : t < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

template <typename T> __device__ __forceinline__ T sqrt_rn(T x);
template <> __device__ __forceinline__ float sqrt_rn<float>(float x) { return __fsqrt_rn(x); }
template <> __device__ __forceinline__ double sqrt_rn<double>(double x) { return __dsqrt_rn(x); }

// audio_track.levels_from_sums up to the rms: mean = T(sum / n) with the division in fp64, rms = sqrt(mean) in T.
template <typename T>
__device__ __forceinline__ bool window_silent(const WalkArgs& a, const void* __restrict__ sums, int k, int64_t count) {
    const T sum = static_cast<const T*>(sums)[k];
    const T mean = (T)((double)sum / (double)count);
    const T rms = sqrt_rn<T>(mean);
    return rms > T(0) ? (double)rms < a.rms_cut : a.silent_without_rms != 0;
}

// One step of the walk from st.current_start, by one thread.  Leaves st.status RUNNING, or says why the walk ended.
__device__ void walk_step(const WalkArgs& a, hmm_segment_walk_state& st, const void* __restrict__ sums,
                          hmm_segment_record* __restrict__ records) {
    const double start = st.current_start;
    const StepSpan sp = step_span(a, start);
    st.steps += 1;
    double optimal_end = sp.end;
    hmm_segment_record rec;
    rec.first_frame = 0;
    rec.last_frame = -1;
    rec.cut_pair = -1;
    rec.cut_window = -1;
    rec.pairs_consulted = 0;
    rec.windows_consulted = 0;
    if (a.n_frames > 0) {
        rec.first_frame = time_bound(a.times, a.n_frames, start, false);
        const int last = time_bound(a.times, a.n_frames, sp.end, true) - 1;
        for (int k = last; k > rec.first_frame; --k) {                       // pair k - 1 = (frame k, frame k - 1), from the end
            rec.pairs_consulted += 1;
            if (a.flags[k - 1] != 0) {
                st.status = HMM_SEGMENT_WALK_FLAGGED;
                st.flagged_pair = k - 1;
                return;
            }
            if (a.scores[k - 1] < a.sim_threshold) {
                optimal_end = a.times[k];
                rec.cut_pair = k - 1;
                break;
            }
        }
    }
    if (a.has_audio) {
        if (sp.n_windows > a.max_windows) {                                  // the table could not hold this step
            st.status = HMM_SEGMENT_WALK_BOUND;
            return;
        }
        for (int k = 0; k < (int)sp.n_windows; ++k) {
            rec.windows_consulted += 1;
            const int64_t at = sp.S + sp.first_off - (int64_t)k * a.window;
            const int64_t lo = at < a.track_len ? at : a.track_len;
            const int64_t count = (at + a.window < a.track_len ? at + a.window : a.track_len) - lo;
            const bool silent = a.track_f64 ? window_silent<double>(a, sums, k, count) : window_silent<float>(a, sums, k, count);
            if (silent) {
                optimal_end = (double)at / (double)a.sample_rate;            // lo / audio_sample_rate: both exact in fp64
                rec.cut_window = k;
                break;
            }
        }
    }
    if (optimal_end - start < a.min_dur) optimal_end = py_min(start + a.min_dur, a.total);
    const int n = st.n_segments;
    if (n < 0 || n >= a.max_steps) {
        st.status = HMM_SEGMENT_WALK_BOUND;
        return;
    }
    rec.start_time = start;
    rec.end_time = optimal_end;
    if (a.n_frames > 0) rec.last_frame = time_bound(a.times, a.n_frames, optimal_end, true) - 1;
    if (rec.last_frame < rec.first_frame) rec.last_frame = rec.first_frame - 1;
    records[n] = rec;
    st.n_segments = n + 1;
    st.current_start = optimal_end;
    if (!(optimal_end < a.total)) st.status = HMM_SEGMENT_WALK_DONE;         // while current_start < total_duration
}

__device__ __forceinline__ hmm_segment_walk_state walk_begin(const WalkArgs& a) {
    hmm_segment_walk_state st;
    st.n_segments = 0;
    st.status = 0.0 < a.total ? HMM_SEGMENT_WALK_RUNNING : HMM_SEGMENT_WALK_DONE;
    st.flagged_pair = -1;
    st.steps = 0;
    st.current_start = 0.0;
    return st;
}

// No audio: the whole walk.
__global__ __launch_bounds__(kWave) void segment_walk_video_kernel(WalkArgs a, hmm_segment_walk_state* state,
                                                                   hmm_segment_record* __restrict__ records) {
    if (threadIdx.x != 0) return;
    hmm_segment_walk_state st = walk_begin(a);
    for (int step = 0; step < a.max_steps && st.status == HMM_SEGMENT_WALK_RUNNING; ++step) walk_step(a, st, nullptr, records);
    if (st.status == HMM_SEGMENT_WALK_RUNNING) st.status = HMM_SEGMENT_WALK_BOUND;
    *state = st;
}

// With audio: the state, and the window table of step 0.
__global__ __launch_bounds__(kWalkThreads) void segment_walk_plan_kernel(WalkArgs a, hmm_segment_walk_state* state,
                                                                         int64_t* __restrict__ table) {
    __shared__ StepSpan s_span;
    __shared__ int s_running;
    if (threadIdx.x == 0) {
        const hmm_segment_walk_state st = walk_begin(a);
        *state = st;
        s_running = st.status == HMM_SEGMENT_WALK_RUNNING;
        s_span = step_span(a, st.current_start);
    }
    __syncthreads();
    write_table(a, s_span, s_running != 0, table);
}

// With audio: one step from the sums of its windows, then the table of the next step (all lengths 0 when the walk ends here; a
// launch that finds the walk ended already leaves the table, which is zero by then, alone).
__global__ __launch_bounds__(kWalkThreads) void segment_walk_decide_kernel(WalkArgs a, hmm_segment_walk_state* state,
                                                                           hmm_segment_record* __restrict__ records,
                                                                           int64_t* table, const void* sums, int last_step) {
    __shared__ StepSpan s_span;
    __shared__ int s_running, s_stepped;
    if (threadIdx.x == 0) {
        hmm_segment_walk_state st = *state;
        s_stepped = st.status == HMM_SEGMENT_WALK_RUNNING;
        if (s_stepped) {
            walk_step(a, st, sums, records);
            if (last_step && st.status == HMM_SEGMENT_WALK_RUNNING) st.status = HMM_SEGMENT_WALK_BOUND;
            *state = st;
        }
        s_running = st.status == HMM_SEGMENT_WALK_RUNNING;
        s_span = step_span(a, st.current_start);
    }
    __syncthreads();
    if (s_stepped) write_table(a, s_span, s_running != 0, table);
}

static size_t walk_table_bytes(int max_windows) { return align_up((size_t)max_windows * 2 * sizeof(int64_t), 256); }

}  // namespace hmm

using namespace hmm;

extern "C" size_t hmm_segment_walk_workspace_bytes(int max_windows, int max_steps) {
    if (max_windows <= 0 || max_steps <= 0) return 0;
    return walk_table_bytes(max_windows) + align_up((size_t)max_windows * sizeof(double), 256);
}

// Both entry points.  who: the name the refusals carry.  pcm16: the track holds int16 samples (track_dtype is then not looked at); its
// sums are fp64 -- exact, the bits of the fp64 track of x / 32768.0 (audio_track.hip) -- so mean and rms are formed as for fp64.
#define WALK_REQUIRE(cond, code, fmt, ...) HMM_REQUIRE(cond, code, "%s: " fmt, who, ##__VA_ARGS__)

static int segment_walk(const char* who, bool pcm16, const double* scores_dev, const int32_t* flags_dev, const double* times_dev,
                        const double* times_host, int n_frames, const void* track_dev, int track_dtype, int64_t track_len,
                        int sample_rate, double total_duration, double max_segment_duration, double min_segment_duration,
                        double frame_similarity_threshold, double rms_cut, int silent_without_rms, int max_windows, int max_steps,
                        hmm_segment_record* records_out_dev, hmm_segment_walk_state* state_out_dev, void* workspace_dev,
                        size_t workspace_bytes, hmm_stream_t stream) {
    const bool has_audio = track_dev != nullptr;
    WALK_REQUIRE(records_out_dev && state_out_dev, HMM_E_INVALID, "null pointer (records or state)");
    WALK_REQUIRE(n_frames >= 0, HMM_E_INVALID, "n_frames=%d is negative", n_frames);
    WALK_REQUIRE(n_frames == 0 || (times_dev && times_host), HMM_E_INVALID, "null pointer (times of %d frames)", n_frames);
    WALK_REQUIRE(n_frames <= 1 || (scores_dev && flags_dev), HMM_E_INVALID, "null pointer (scores or flags of %d pairs)",
                n_frames - 1);
    WALK_REQUIRE(!has_audio || workspace_dev, HMM_E_INVALID, "null pointer (workspace of a walk with audio)");
    WALK_REQUIRE(std::isfinite(total_duration) && std::isfinite(max_segment_duration) && std::isfinite(min_segment_duration),
                HMM_E_INVALID, "total_duration, max_segment_duration or min_segment_duration is not finite");
    WALK_REQUIRE(frame_similarity_threshold == frame_similarity_threshold && rms_cut == rms_cut, HMM_E_INVALID,
                "frame_similarity_threshold or rms_cut is NaN");
    WALK_REQUIRE(min_segment_duration > 0.0, HMM_E_INVALID, "min_segment_duration=%g must be positive (the walk would not end)",
                min_segment_duration);
    WALK_REQUIRE(max_steps >= 1 && max_windows >= 0, HMM_E_INVALID, "max_steps=%d, max_windows=%d: need max_steps >= 1 and "
                "max_windows >= 0", max_steps, max_windows);
    for (int i = 0; i < n_frames; ++i) {
        WALK_REQUIRE(std::isfinite(times_host[i]), HMM_E_INVALID, "time of frame %d is not finite", i);
        WALK_REQUIRE(i == 0 || times_host[i - 1] <= times_host[i], HMM_E_INVALID,
                    "frame times are unsorted: frame %d at %.17g follows %.17g", i, times_host[i], times_host[i - 1]);
    }
    if (has_audio) {
        WALK_REQUIRE(pcm16 || track_dtype == 0 || track_dtype == 1, HMM_E_INVALID, "track_dtype must be 0 (fp32) or 1 (fp64), got %d",
                     track_dtype);
        WALK_REQUIRE(!pcm16 || (int64_t)(0.5 * (double)sample_rate) <= kPcmWindowMax, HMM_E_INVALID,
                     "a window of 0.5 * sample_rate = %lld samples is above 4194304 (2^22): its sum is no longer exact",
                     (long long)(0.5 * (double)sample_rate));
        WALK_REQUIRE(track_len >= 0 && sample_rate >= 2 && max_windows >= 1, HMM_E_INVALID,
                    "audio needs track_len >= 0, sample_rate >= 2 and max_windows >= 1 (track_len=%lld, sample_rate=%d, "
                    "max_windows=%d)", (long long)track_len, sample_rate, max_windows);
        WALK_REQUIRE(total_duration * (double)sample_rate < 4503599627370496.0, HMM_E_INVALID,
                    "total_duration * sample_rate = %g does not stay below 2^52 samples", total_duration * (double)sample_rate);
    }
    WALK_REQUIRE(((uintptr_t)records_out_dev & 7) == 0 && ((uintptr_t)state_out_dev & 7) == 0 && ((uintptr_t)workspace_dev & 7) == 0 &&
                    ((uintptr_t)scores_dev & 7) == 0 && ((uintptr_t)times_dev & 7) == 0 && ((uintptr_t)flags_dev & 3) == 0 &&
                    ((uintptr_t)track_dev & 15) == 0, HMM_E_INVALID,
                "misaligned pointer (records, state, workspace, scores and times 8-byte aligned, flags 4, the track 16)");
    const size_t need = has_audio ? hmm_segment_walk_workspace_bytes(max_windows, max_steps) : 0;
    WALK_REQUIRE(workspace_bytes >= need, HMM_E_WORKSPACE, "workspace of %zu bytes, %zu needed", workspace_bytes, need);
    if (pcm16 && has_audio) {                                                // what the call writes may not lie in the track's bytes
        const uint64_t t0 = (uint64_t)(uintptr_t)track_dev, t1 = t0 + (uint64_t)track_len * 2;
        const auto inside = [&](const void* p, uint64_t bytes) {
            const uint64_t q = (uint64_t)(uintptr_t)p;
            return bytes != 0 && t1 > t0 && q < t1 && t0 < q + bytes;
        };
        WALK_REQUIRE(!inside(records_out_dev, (uint64_t)max_steps * sizeof(hmm_segment_record)) &&
                         !inside(state_out_dev, sizeof(hmm_segment_walk_state)) && !inside(workspace_dev, need),
                     HMM_E_INVALID, "the records, the state or the workspace overlaps the track");
    }

    WalkArgs a;
    a.scores = scores_dev;
    a.flags = flags_dev;
    a.times = times_dev;
    a.n_frames = n_frames;
    a.has_audio = has_audio ? 1 : 0;
    a.track_f64 = pcm16 || track_dtype == 1;
    a.track_len = track_len;
    a.sample_rate = sample_rate;
    a.window = (int64_t)(0.5 * (double)sample_rate);                         // int(0.5 * audio_sample_rate)
    a.total = total_duration;
    a.max_dur = max_segment_duration;
    a.min_dur = min_segment_duration;
    a.sim_threshold = frame_similarity_threshold;
    a.rms_cut = rms_cut;
    a.silent_without_rms = silent_without_rms != 0;
    a.max_windows = has_audio ? max_windows : 0;
    a.max_steps = max_steps;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!has_audio) {
        segment_walk_video_kernel<<<1, kWave, 0, st>>>(a, state_out_dev, records_out_dev);
        HMM_LAUNCH_CHECK();
        return HMM_OK;
    }
    int64_t* table = static_cast<int64_t*>(workspace_dev);
    void* sums = static_cast<char*>(workspace_dev) + walk_table_bytes(max_windows);
    segment_walk_plan_kernel<<<1, kWalkThreads, 0, st>>>(a, state_out_dev, table);
    HMM_LAUNCH_CHECK();
    for (int step = 0; step < max_steps; ++step) {
        if (pcm16) launch_pcm16_window_sums(track_dev, track_len, table, max_windows, static_cast<double*>(sums), st);
        else launch_window_sums(track_dev, track_dtype, track_len, table, max_windows, sums, st);
        HMM_LAUNCH_CHECK();
        segment_walk_decide_kernel<<<1, kWalkThreads, 0, st>>>(a, state_out_dev, records_out_dev, table, sums, step == max_steps - 1);
        HMM_LAUNCH_CHECK();
    }
    return HMM_OK;
}
#undef WALK_REQUIRE

extern "C" int hmm_segment_walk(const double* scores_dev, const int32_t* flags_dev, const double* times_dev, const double* times_host,
                                int n_frames, const void* track_dev, int track_dtype, int64_t track_len, int sample_rate,
                                double total_duration, double max_segment_duration, double min_segment_duration,
                                double frame_similarity_threshold, double rms_cut, int silent_without_rms, int max_windows,
                                int max_steps, hmm_segment_record* records_out_dev, hmm_segment_walk_state* state_out_dev,
                                void* workspace_dev, size_t workspace_bytes, hmm_stream_t stream) {
    return segment_walk("segment_walk", false, scores_dev, flags_dev, times_dev, times_host, n_frames, track_dev, track_dtype, track_len,
                        sample_rate, total_duration, max_segment_duration, min_segment_duration, frame_similarity_threshold, rms_cut,
                        silent_without_rms, max_windows, max_steps, records_out_dev, state_out_dev, workspace_dev, workspace_bytes, stream);
}

extern "C" int hmm_segment_walk_pcm16(const double* scores_dev, const int32_t* flags_dev, const double* times_dev,
                                      const double* times_host, int n_frames, const void* track_dev, int64_t track_len, int sample_rate,
                                      double total_duration, double max_segment_duration, double min_segment_duration,
                                      double frame_similarity_threshold, double rms_cut, int silent_without_rms, int max_windows,
                                      int max_steps, hmm_segment_record* records_out_dev, hmm_segment_walk_state* state_out_dev,
                                      void* workspace_dev, size_t workspace_bytes, hmm_stream_t stream) {
    return segment_walk("segment_walk_pcm16", true, scores_dev, flags_dev, times_dev, times_host, n_frames, track_dev, 1, track_len,
                        sample_rate, total_duration, max_segment_duration, min_segment_duration, frame_similarity_threshold, rms_cut,
                        silent_without_rms, max_windows, max_steps, records_out_dev, state_out_dev, workspace_dev, workspace_bytes, stream);
}
