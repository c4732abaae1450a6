// The decision loop of extract_frames_from_video (hippomm/core/batch_process.py:179-228) on gfx950: for every candidate frame of a
// batch, in order, "is it far enough from the last saved frame to be saved?", with the last saved frame (the anchor), the running
// cumulative difference and the time of the last save resident on the device, so a batch needs one upload, one launch sequence and
// one read-back.
//
// The loop is ordered -- the anchor moves whenever a frame is saved -- so each candidate gets two launches on the caller's in-order
// stream: the SSIM tile kernel against whatever slot the state names as the anchor, and a one-workgroup decide kernel that sums the
// tile partials, applies the reference's rules (:188-218) in fp64 and updates the state.  Nothing waits for another workgroup: the
// order is the stream's.  The tile body and the fixed-order sum are ssim.hip's (ssim_core.h), so a compared candidate's diff is
// 1.0 - hmm_ssim_pairs(candidate, anchor, data_range 255) bit for bit.
#include "hmm_common.h"
#include "ssim_core.h"

#include <cmath>

#pragma clang fp contract(off)

namespace hmm {

constexpr int kCarryThreads = 256;
constexpr int kCarryBlocks = 512;

__device__ __forceinline__ int clamp_slot(int slot, int n_slots) { return min(max(slot, 0), n_slots - 1); }

// What the reference's `elif current_time - last_save_time >= 1.0: if frame_count % check_interval == 0:` admits to a comparison.
__device__ __forceinline__ bool walk_eligible(const hmm_extract_state& st, int check, double time, double min_gap) {
    return st.has_anchor != 0 && check != 0 && (time - st.last_save_time >= min_gap);
}

// One workgroup per tile of the candidate `slot` against the state's anchor slot; every workgroup reads the state (written by
// the previous candidate's decide kernel, an earlier launch on the same stream) and leaves at once when nothing is to be compared.
__global__ __launch_bounds__(kSsimTW) void extract_tile_kernel(const uint8_t* __restrict__ gray, int n_slots, int H, int W, int slot,
                                                               double time, int check, double min_gap,
                                                               const hmm_extract_state* state, int tiles_x,
                                                               double* __restrict__ partial) {
    __shared__ SsimTileLds s;
    const hmm_extract_state st = *state;
    if (!walk_eligible(st, check, time, min_gap)) return;
    const int tile = blockIdx.x;
    const int x0 = (tile % tiles_x) * kSsimTW, y0 = (tile / tiles_x) * kSsimTH;
    const int64_t hw = (int64_t)H * W;
    const int anchor = clamp_slot(st.anchor_slot, n_slots);
    ssim_tile_partial(gray + slot * hw, gray + anchor * hw, H, W, x0, y0, 255.0, s, partial + tile);
}

// One workgroup: the fixed-order sum of the partials (the order of ssim_finish_kernel), then lines :188-218 of the reference.
__global__ __launch_bounds__(kFinishThreads) void extract_decide_kernel(const double* __restrict__ partial, int n_tiles, double count,
                                                                        int slot, double time, int check, int deny,
                                                                        double threshold, double min_gap, hmm_extract_state* state,
                                                                        hmm_extract_record* record) {
    __shared__ double s_wave[kFinishThreads / kWave];
    __shared__ int s_compare;
    hmm_extract_state st = {};
    if (threadIdx.x == 0) {                                                // thread 0 alone reads the state, and later writes it
        st = *state;
        s_compare = walk_eligible(st, check, time, min_gap) ? 1 : 0;
    }
    __syncthreads();
    const bool compare = s_compare != 0;                                   // uniform over the workgroup
    double sum = 0.0;
    if (compare) sum = ssim_partials_sum(partial, n_tiles, s_wave);
    if (threadIdx.x != 0) return;
    double diff = 0.0;
    bool save = st.has_anchor == 0;                                        // "always save first frame"
    if (compare) {
        const double score = sum / count;
        diff = 1.0 - score;
        st.cumulative_diff += diff;
        save = diff > threshold || st.cumulative_diff > threshold;
    }
    const bool saved = save && !deny;
    if (saved) {
        st.has_anchor = 1;
        st.anchor_slot = slot;
        st.cumulative_diff = 0.0;
        st.last_save_time = time;
    }
    *state = st;
    hmm_extract_record rec;
    rec.compared = compare ? 1 : 0;
    rec.saved = saved ? 1 : 0;
    rec.anchor_slot_after = st.anchor_slot;
    rec.has_anchor_after = st.has_anchor;
    rec.diff = diff;
    rec.cumulative_after = st.cumulative_diff;
    rec.last_save_time_after = st.last_save_time;
    *record = rec;
}

// gray[0] = gray[anchor] when the state has an anchor outside slot 0.  T = uint4 when a frame is a whole number of 16-byte words.
template <typename T>
__global__ __launch_bounds__(kCarryThreads) void extract_carry_copy_kernel(uint8_t* gray, int n_slots, int64_t words_per_frame,
                                                                           const hmm_extract_state* state) {
    const hmm_extract_state st = *state;
    if (st.has_anchor == 0) return;
    const int anchor = clamp_slot(st.anchor_slot, n_slots);
    if (anchor == 0) return;
    const T* src = reinterpret_cast<const T*>(gray) + anchor * words_per_frame;
    T* dst = reinterpret_cast<T*>(gray);
    for (int64_t i = (int64_t)blockIdx.x * kCarryThreads + threadIdx.x; i < words_per_frame; i += (int64_t)gridDim.x * kCarryThreads)
        dst[i] = src[i];
}

// After the copy (its own launch: every workgroup of the copy has read the old slot by then).
__global__ void extract_carry_set_kernel(hmm_extract_state* state) {
    if (threadIdx.x == 0 && blockIdx.x == 0 && state->has_anchor != 0) state->anchor_slot = 0;
}

}  // namespace hmm

using namespace hmm;

extern "C" size_t hmm_extract_walk_workspace_bytes(int H, int W) {
    if (H < 7 || W < 7) return 0;
    return align_up((size_t)ssim_tiles(H, W, nullptr) * sizeof(double), 256);
}

extern "C" int hmm_extract_walk(const uint8_t* gray_slots_dev, int n_slots, int H, int W, int first_slot, int count,
                                const double* times_host, const int32_t* check_host, const int32_t* deny_host,
                                double max_diff_threshold, double min_gap, hmm_extract_state* state_dev,
                                hmm_extract_record* records_out_dev, void* workspace_dev, size_t workspace_bytes,
                                hmm_stream_t stream) {
    HMM_REQUIRE(gray_slots_dev && times_host && check_host && deny_host && state_dev && records_out_dev && workspace_dev,
                HMM_E_INVALID, "extract_walk: null pointer");
    HMM_REQUIRE(H >= 7 && W >= 7, HMM_E_INVALID, "extract_walk: win_size exceeds image extent (%dx%d frames, 7x7 window)", H, W);
    HMM_REQUIRE(n_slots >= 2 && count >= 1, HMM_E_INVALID, "extract_walk: n_slots=%d count=%d, need n_slots >= 2 and count >= 1",
                n_slots, count);
    HMM_REQUIRE(first_slot >= 1 && (int64_t)first_slot + count <= n_slots, HMM_E_INVALID,
                "extract_walk: candidates %d .. %lld outside slots 1 .. %d", first_slot, (long long)first_slot + count - 1,
                n_slots - 1);
    HMM_REQUIRE(((uintptr_t)state_dev & 7) == 0 && ((uintptr_t)records_out_dev & 7) == 0 && ((uintptr_t)workspace_dev & 7) == 0,
                HMM_E_INVALID, "extract_walk: state, records and workspace must be 8-byte aligned");
    HMM_REQUIRE(max_diff_threshold == max_diff_threshold && min_gap == min_gap, HMM_E_INVALID,
                "extract_walk: max_diff_threshold or min_gap is NaN");
    for (int i = 0; i < count; ++i)
        HMM_REQUIRE(std::isfinite(times_host[i]), HMM_E_INVALID, "extract_walk: time of candidate %d is not finite", i);
    HMM_REQUIRE(workspace_bytes >= hmm_extract_walk_workspace_bytes(H, W), HMM_E_WORKSPACE,
                "extract_walk: workspace of %zu bytes, %zu needed", workspace_bytes, hmm_extract_walk_workspace_bytes(H, W));
    hipStream_t st = static_cast<hipStream_t>(stream);
    int tiles_x = 0;
    const int n_tiles = ssim_tiles(H, W, &tiles_x);
    double* partial = static_cast<double*>(workspace_dev);
    const double positions = (double)(H - 6) * (double)(W - 6);
    for (int i = 0; i < count; ++i) {
        const int slot = first_slot + i;
        const int check = check_host[i] != 0, deny = deny_host[i] != 0;
        extract_tile_kernel<<<(unsigned)n_tiles, kSsimTW, 0, st>>>(gray_slots_dev, n_slots, H, W, slot, times_host[i], check, min_gap,
                                                                   state_dev, tiles_x, partial);
        HMM_LAUNCH_CHECK();
        extract_decide_kernel<<<1, kFinishThreads, 0, st>>>(partial, n_tiles, positions, slot, times_host[i], check, deny,
                                                            max_diff_threshold, min_gap, state_dev, records_out_dev + i);
        HMM_LAUNCH_CHECK();
    }
    return HMM_OK;
}

extern "C" int hmm_extract_carry(uint8_t* gray_slots_dev, int n_slots, int H, int W, hmm_extract_state* state_dev,
                                 hmm_stream_t stream) {
    HMM_REQUIRE(gray_slots_dev && state_dev, HMM_E_INVALID, "extract_carry: null pointer");
    HMM_REQUIRE(n_slots >= 1 && H >= 1 && W >= 1, HMM_E_INVALID, "extract_carry: bad shape n_slots=%d H=%d W=%d", n_slots, H, W);
    HMM_REQUIRE(((uintptr_t)state_dev & 7) == 0, HMM_E_INVALID, "extract_carry: state must be 8-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t hw = (int64_t)H * W;
    if (hw % 16 == 0 && ((uintptr_t)gray_slots_dev & 15) == 0) {
        const int64_t words = hw / 16;
        const unsigned grid = (unsigned)std::min<int64_t>((words + kCarryThreads - 1) / kCarryThreads, kCarryBlocks);
        extract_carry_copy_kernel<uint4><<<grid, kCarryThreads, 0, st>>>(gray_slots_dev, n_slots, words, state_dev);
    } else {
        const unsigned grid = (unsigned)std::min<int64_t>((hw + kCarryThreads - 1) / kCarryThreads, kCarryBlocks);
        extract_carry_copy_kernel<uint8_t><<<grid, kCarryThreads, 0, st>>>(gray_slots_dev, n_slots, hw, state_dev);
    }
    HMM_LAUNCH_CHECK();
    extract_carry_set_kernel<<<1, 64, 0, st>>>(state_dev);
    HMM_LAUNCH_CHECK();
    return HMM_OK;
}
