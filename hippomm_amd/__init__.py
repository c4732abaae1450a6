"""hippomm_amd -- MI355X-native (gfx950) hot path of HippoMM.

Host-side mirror of the three reference call sites, bound to hand-written HIP kernels
through the C ABI in include/hippomm_hip.h:

    hippomm_amd.encoder.ImageBind                    <- hippomm/models/foundation_models.py:21-151
    hippomm_amd.consolidation._select_key_frames     <- hippomm/core/hippocampal_memory.py:944-967
    hippomm_amd.consolidation.KeyFrameSelector       the same selection grown batch by batch (live path, :1290-1365)
    hippomm_amd.vector_ops.top_k_cosine_similarity   <- hippomm/utils/vector_ops.py:151-188

and the two SSIM call sites of the formation path (frame SSIM in hippomm_amd/csrc/ssim.hip; a module per stage of the frame path
-- ssim, resize, frame_cache, frame_extraction, segmentation -- and every public name of theirs still imports from
hippomm_amd.segmentation, where all of them used to live):

    hippomm_amd.ssim.compute_frame_difference           <- hippomm/core/batch_process.py:32-69
    hippomm_amd.segmentation._compute_frame_similarity  <- hippomm/core/hippocampal_memory.py:980-991
    hippomm_amd.segmentation._segment_sequence          <- hippomm/core/hippocampal_memory.py:1002-1114
    hippomm_amd.sharding                             one-process-per-GPU sharding (RCCL all-gather)

and the audio of a whole video in one call (clip gather, peak normalisation and resampling in hippomm_amd/csrc/audio_track.hip):

    hippomm_amd.audio_track.AudioTrack, ImageBind.extract_audio_segments  <- hippomm/core/hippocampal_memory.py:1198-1251

and a baseline JPEG decoder with the pixel work on the GPU, bit-exact with Pillow (hippomm_amd/csrc/jpeg.hip):

    hippomm_amd.decode_jpeg                          <- Image.open(path).convert("RGB") of the reference's frame reads

and its counterpart, a baseline JPEG encoder on the GPU, byte for byte Pillow's file (hippomm_amd/csrc/jpeg_encode.hip):

    hippomm_amd.encode_jpeg                          <- Image.fromarray(rgb).save(buf, "JPEG", quality=q, subsampling=s)
    hippomm_amd.frame_extraction.save_frame, save_frames <- hippomm/core/batch_process.py:73-114 (cv2.imwrite)

and, opt-in, the decoded pixels of the frames just saved kept on the device for the two reads that follow (hmm_jpeg_encoded_pixels):

    save_frames(..., cache=FrameCache, tower_inputs=preprocess.TowerInputCache), ImageBind(..., tower_inputs=)

and the callers' retrieval step with the reference's row and fallback rules applied on the device (hmm_rank_segment_hits_filtered):

    hippomm_amd.find_relevant_video_segments         <- hippomm/core/hippocampal_memory.py:3127-3279
    hippomm_amd.find_relevant_audio_segments         <- hippomm/core/hippocampal_memory.py:3281-3383

and the step right after it, the frame windows read around every frame_time of the relevant segments: cv2.resize's 8-bit
INTER_LINEAR for targets no larger than the source (hippomm_amd/csrc/resize.hip), the JPEG and the SSIM dedup in one pass, without
a file round-trip (video decoding stays with the caller; the time of a question is the caller's seeks and the captioner, not this):

    hippomm_amd.recall_window_frames                 <- hippomm/core/hippocampal_memory.py:2226-2249, :2789-2812
    hippomm_amd.resize.resize_frames                 <- cv2.resize(frame, (320, 180))

and, opt-in, the feature matrices of an event file written as JSON text on the device, byte for byte json.dump's (hippomm_amd/csrc/event_json.hip):

    hippomm_amd.event_store.save_event(..., matrices="device"), event_json_bytes, matrix_json_bytes  <- hippomm/core/hippocampal_memory.py:331-335

and, opt-in too, read back from that text on the device, the bits of np.array(json.load(f)) (hippomm_amd/csrc/event_json_parse.hip):

    hippomm_amd.event_store.parse_matrix_device, parse_event_features(..., matrices="device"),
    build_event_store / refresh_event_store(..., parse="device")                                   <- hippomm/core/hippocampal_memory.py:369-395

and the decision loop of frame extraction with the last saved frame, the cumulative difference and the time of the last save on the
device: each frame uploaded once, one read-back per batch of candidates (hippomm_amd/csrc/extract_walk.hip):

    hippomm_amd.extract_frames, FrameExtractor, extraction_records  <- hippomm/core/batch_process.py:179-228

and the step that joins formation to the stored event, a video's segment memories consolidated into one: the stacked, time-ordered
matrix gathered on the device from the segments' blocks where they lie (hippomm_amd/csrc/rows_gather.hip), the selection on it,
nothing read back but the kept list, and a result that can stay a device tensor:

    hippomm_amd.consolidate_short_term_memory        <- hippomm/core/hippocampal_memory.py:754-927

and, opt-in, the window walk of sequence segmentation itself on the device over resident pair scores, frame times and the audio
track, the segment list the one read-back (hippomm_amd/csrc/segment_walk.hip):

    hippomm_amd.segmentation.segment_sequence(..., walk="device"), frame_cache.PathScorer.score_adjacent  <- hippomm/core/hippocampal_memory.py:1002-1114
"""
__version__ = "0.1.0"

from .consolidation import consolidate_short_term_memory  # noqa: E402,F401
from .jpeg import decode_jpeg, encode_jpeg  # noqa: E402,F401
from .frame_extraction import FrameExtractor, extract_frames, extraction_records  # noqa: E402,F401
from . import segmentation  # noqa: E402,F401  (before retrieval: it re-exports retrieval's recall walk, which needs its SequenceSegment)
from .retrieval import (feature_entries, find_relevant_audio_segments, find_relevant_video_segments,  # noqa: E402,F401
                        recall_window_frames)
