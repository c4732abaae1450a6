// The launch of window_sums_kernel (audio_track.hip), for the two entry points that need a window's sum of squares in numpy's
// order: hmm_audio_window_sums and the per-step launch of hmm_segment_walk (segment_walk.hip).  One kernel, one set of bits.
// Likewise pcm16_window_sums_kernel for a 16-bit track: hmm_audio_pcm16_window_sums and hmm_segment_walk_pcm16.
#pragma once
#include "hmm_common.h"

namespace hmm {

// One workgroup per row of windows_dev (n_windows x (start, length) int64, clamped to the track by the kernel); sums_dev[w] in the
// track's dtype.  n_windows >= 1.  Nothing is validated here: the entry points have done that.
void launch_window_sums(const void* track_dev, int track_dtype, int64_t track_len, const int64_t* windows_dev, int n_windows,
                        void* sums_dev, hipStream_t stream);

// The longest window of a 16-bit track: up to here the fp64 sum of (x / 32768)^2 is exact in any order (audio_track.hip).
constexpr int64_t kPcmWindowMax = (int64_t)1 << 22;

// The same for a track of int16 samples: sums_dev[w] the fp64 sum of (x / 32768)^2, exact; the kernel clamps a row to the track and
// its length to kPcmWindowMax.
void launch_pcm16_window_sums(const void* track_dev, int64_t track_len, const int64_t* windows_dev, int n_windows, double* sums_dev,
                              hipStream_t stream);

}  // namespace hmm
