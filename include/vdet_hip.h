/*
 * vdet_hip.h -- C-ABI of libvdet_hip.so: the MI355X (gfx950) implementation of vdetlib's
 * per-frame scoring / tubelet post-processing hot path.
 *
 * This is the drop-in boundary.  The reference's only native component is the Cython module
 * utils/cython_nms (built from utils/nms.pyx by setup.py:8-14); its three entry points are what
 * vdet_nms_f32 / vdet_track_det_nms_f32 replace.  The remaining entry points are the array forms
 * of the numeric cores of vdet/video_det.py, vdet/track.py, vdet/tubelet_cls.py and
 * utils/common.py:iou, so that T-CNN style host code (vdetlib_amd/, a py3 mirror of the reference's
 * python API) never computes on the CPU.  Reference citations are file:line in /root/reference.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types, no exceptions across the boundary.
 *   - The caller owns every buffer.  "h_" parameters are host pointers, "d_" parameters are device
 *     pointers on the context's GPU.  The library never frees caller memory; device scratch is
 *     owned by the vdet_ctx.
 *   - Every function returns VDET_OK (0) or a negative vdet_status.  vdet_last_error() gives text.
 *   - h_* entry points are synchronous.  d_* entry points enqueue on the context's stream and
 *     return; data-dependent failures (capacity overflow, zero union) are latched on the device
 *     and reported by vdet_sync().
 *   - A context is not thread-safe: one per thread / per GPU (reference is single-threaded, GIL
 *     held throughout).  Results are deterministic (no float atomics on any result path).
 *   - Boxes are (x1,y1,x2,y2), inclusive pixel coordinates, +1 convention (utils/nms.pyx:24,61-62).
 *   - Sort order wherever the reference says scores.argsort()[::-1] (utils/nms.pyx:25,80 -- numpy's
 *     default UNSTABLE sort): descending score, ties by DESCENDING original index
 *     (= argsort(kind='stable')[::-1]); -0.0 == +0.0; NaN scores sort first.  A caller-supplied
 *     `order` reproduces any other tie order exactly.
 *
 * Limits (the reference has none of them: its lists and loops are python objects; every limit is an error code, never a
 * crash, and nothing is written out of bounds):
 *   what                                   limit                      beyond it
 *   boxes per frame, every entry point     B <= 32767                 VDET_EINVAL (u16 box indices, bit 15 = zero-union tag)
 *   boxes per frame, d_* volume calls      B <= ~18000                VDET_EINVAL (a (frame, class) argsort lives in the CU's
 *                                                                     160 KiB LDS: 6 B / box + tables); the h_* calls fall
 *                                                                     back to a global bitonic sort up to 32767
 *   regular-frame fast kernels             B <= 17408                 same results through the general kernels (slower)
 *   rows of a volume                       F*C, F*B < 2^31 - 16       VDET_EINVAL
 *   rows of an h_* call                    n < 2^31, <= 32767 / frame VDET_EINVAL
 *   edges of one suppression graph         < 2^32                     VDET_ENOMEM
 *   survivors per (frame, class)           cap (caller's choice)      VDET_ECAP latched, count still written
 *   vdet_det_nms_volume top-k              1 <= topk <= 128           VDET_EINVAL
 *   box decode (vdet_decode_boxes, vdet_det_nms_volume_deltas, vdet_tubelet_dets)   H, W >= 1; rois, deltas and box outputs
 *                                          16-byte aligned; N*K <= 2^40 (vdet_decode_boxes), C*T*F < 2^31 - 16    VDET_EINVAL
 *   RPN proposal layer (vdet_rpn_proposals)  1 <= A <= 64; Hf, Wf >= 1; Hf*Wf*A < 2^24; F*Hf*Wf*A < 2^31 - 16; stride >= 1;
 *                                          1 <= post_nms_top_n <= pre_nms_top_n <= 16384; H, W >= 1; min_size, offset finite;
 *                                          score frame stride >= A*Hf*Wf; d_rois 16-byte aligned    VDET_EINVAL
 *   temporal window / taps                 odd, <= 31                 VDET_EINVAL (the one-pass volume kernel: 3 or 5, other
 *                                                                     windows run the separate kernels)
 *   frames per video, vdet_video_batch     none                       videos of more than 1536 frames re-score their tubelet
 *                                                                     series one thread per series (slower, same results)
 *   single-launch h_* calls                n <= 640 rows, t <= 256    larger inputs take the general kernel chain (same results)
 *   link table up front                    B <= 1024                  larger frames scan link steps on demand (same results)
 *   evaluator: tracks per (frame, class)   T <= 1024                  VDET_EINVAL (vdet_eval_match_tracks[_batch])
 *   evaluator: gt boxes per (video, frame, class)  <= 256             VDET_EINVAL (vdet_eval_gt_upload)
 *   evaluator: gt table cells              videos x frames x K < 2^31 VDET_EINVAL;  class slots 1 <= K <= 65536
 *   evaluator: stream entries              < 2^31 (per add: C*T*F or F*C*cap < 2^31)   VDET_EINVAL
 *   device TCN: layers of a net            1 .. 16                    VDET_EINVAL
 *   device TCN: channels of a layer        1 .. 4096 (inputs: 1 .. 16 assembled channels; 1 .. 16 inputs of up to 4096
 *                                          channels together for vdet_tcn_tracks_wide; any count up to 4096 for
 *                                          vdet_tcn_series_f32); the last layer has 2      VDET_EINVAL
 *   device TCN: kernel size                odd, <= 31                 VDET_EINVAL
 *   device TCN: series length, net width   none                       series whose activations exceed 48 KiB of LDS are tiled
 *                                                                     along the series; nets too wide for a 16-position tile keep
 *                                                                     their activations in global memory (slower, same results)
 *   device TCN / overlap: videos per call  V <= 65535, C*T*F < 2^31   VDET_EINVAL
 *   device interpolation: series per call  <= 4                       VDET_EINVAL
 *   device interpolation: rows, frames, stride  none (V <= 65535, C*T*F < 2^31 on both axes)   VDET_EINVAL; one path for
 *                                                                     every size: the kernel keeps no knot list
 *   device anchor route: slots, frames     C*T*F < 2^31, B <= 32767   VDET_EINVAL; an anchor frame outside 0..F: VDET_EINVAL
 *                                                                     latched (vdet_sync).  One path for every size: a link
 *                                                                     step scans the whole frame
 *   device anchor selection: slots         1 <= top_num <= 1024 per (video, class); <= 128 per (frame, class) in frame mode
 *                                                                     VDET_EINVAL (the evaluator's tracks-per-class limit /
 *                                                                     vdet_det_nms_volume's top-k limit).  One path for every
 *                                                                     top_num: selection by threshold, then a sort of <= top_num
 *   device anchor selection / batch forms  B <= 32767, F*B < 2^31 - 16, V <= 65535 (frame mode: F <= 65535), C*T*F < 2^31
 *                                                                     VDET_EINVAL
 *   device merge: slots, series            C*T*F < 2^31 - 16 for Ta, Tb AND the output's T (Ta + Tb under 'combine'), V <= 65535,
 *                                          1 .. 4 series              VDET_EINVAL; one path for every size
 *   device tubelet NMS: rows per list      top_still + T <= 1024, 1 <= R <= 1024 (the evaluator's tracks-per-(frame, class) limit),
 *                                          C*R*F and C*T*F < 2^31 - 16, B <= 32767, V <= 65535      VDET_EINVAL; one path for
 *                                                                     every size: a wave's LDS follows the call's top_still + T
 *   device tubelet re-scoring              B <= 32767, F*B and C*T*F < 2^31 - 16, V <= 65535, window odd      VDET_EINVAL; videos
 *                                                                     of more than 1536 frames re-score their series one thread
 *                                                                     per series (slower, same results)
 *   device R-CNN windows                   1 <= crop_size S <= 1024, S - 2*padding >= 1, H, W <= 32767, num <= 255 sampled boxes
 *                                          per box, windows < 2^31 - 16, C*T*F < 2^31 - 16      VDET_EINVAL; more present tubelet
 *                                                                     boxes than cap: VDET_ECAP latched (vdet_sync), the count
 *                                                                     still written.  One path for every size
 *   device RoI pooling                     1 <= ph, pw <= 32, 1 <= sampling <= 8, Hf, Wf <= 32767, RoIs < 2^31 - 16,
 *                                          RoIs * ceil(K / 64) ('max') or RoIs * ceil(K*ph*pw / 4096) ('align') < 2^31,
 *                                          C*T*F < 2^31 - 16                                    VDET_EINVAL; the tubelet form's
 *                                                                     cap as for the R-CNN windows.  One path for every size
 *   device pixel tracker                  grid S a multiple of 4 in 4 .. 64, 1 <= radius R <= 16, step >= 1, max_frames >= 0,
 *                                          min_conf finite, H, W <= 32767, C*T*F < 2^31 - 16      VDET_EINVAL; an anchor frame
 *                                                                     outside 0..F, or an anchor box that is not finite, beyond
 *                                                                     2^20, empty or wholly outside the image: VDET_EINVAL latched
 *                                                                     (vdet_sync), the slot written as an empty one.  One path
 *                                                                     for every size
 *   greedy loop with the pixel tracker     the pixel tracker's row with T = max_tracks, and B <= 32767, F*C and F*B < 2^31 - 16
 *                                                                     VDET_EINVAL; an anchor box that cannot be tracked:
 *                                                                     VDET_EINVAL latched (vdet_sync), the slot taken with NaN
 *                                                                     rows, the loop goes on
 *   pixel tracker with scale search        (vdet_track_pixels_scaled, vdet_track_volume_pixels_scaled) the row of the call without
 *                                          the search, and 0 <= scales <= 3, 1 <= scale_step <= 25,
 *                                          0 <= scale_penalty <= 65535                            VDET_EINVAL; bad anchor data as in
 *                                                                     the call without the search.  A level whose box has a side
 *                                                                     below 1 or above 2^21 is skipped, never an error
 *   luma integral image                    (vdet_luma_integral) H, W <= 32767, H*W <= 2^24 (255 * H * W fits in 32 bits),
 *                                          F*H/4 and F*ceil((W+1)/128) < 2^31 - 16                VDET_EINVAL.  One path for every size
 *   pixel tracker with box sampling        (vdet_track_pixels_box, vdet_track_volume_pixels_box) the row of the call with the
 *                                          scale search (scales = 0 allowed), and H*W <= 2^24, a non-NULL integral
 *                                                                     VDET_EINVAL; bad anchor data as in the call with point
 *                                                                     sampling.  A cell outside the image or narrower than a
 *                                                                     pixel is a single column / row, never an error
 *   pixel tracker with template update     (vdet_track_pixels_adaptive, vdet_track_volume_pixels_adaptive) the row of the call with
 *                                          the scale search (scales = 0 allowed; box = 1: the row with box sampling), and
 *                                          box 0 or 1, 0 <= update <= 256, update_conf and drift_conf finite
 *                                                                     VDET_EINVAL; bad anchor data as in the siblings.  A
 *                                                                     confidence no step reaches (2.0) is the fixed template,
 *                                                                     never an error
 *   block-motion field                     (vdet_motion_field) block 8, 16 or 32, 1 <= radius <= 16, H, W <= 32767, every output
 *                                          below 2^31 - 16 elements (the largest: 2*F*(Hb+1)*(Wb+1)*2)      VDET_EINVAL.  One path
 *                                                                     for every size
 *   summed table of a motion field         (vdet_motion_table) 1 <= Hb, Wb <= 4096, 2*F*(Hb+1)*(Wb+1)*2 < 2^31 - 16      VDET_EINVAL
 *   propagation of detections              (vdet_propagate_boxes) the motion field's row for block, H, W, Hb, Wb, and
 *                                          1 <= top <= kcap, 1 <= reach <= 16, 2*reach*top <= 1024 (vdet_nms_tracks' list limit),
 *                                          B <= 32767, C*T*F < 2^31 - 16, decay finite and >= 0      VDET_EINVAL; a keep_cnt
 *                                                                     outside 0..kcap, a read keep_idx outside 0..B-1, a source
 *                                                                     box that is not finite or beyond 2^20: VDET_EINVAL latched
 *                                                                     (vdet_sync), the source writes NaN rows.  One path for
 *                                                                     every size
 *   multi-context suppression              (vdet_context_classes, vdet_suppress_context) F*B < 2^31 - 16, C <= 2^31 - 65536,
 *                                          every video below 2^32 scores (32-bit counters), at most 65535 videos, ratio in
 *                                          (0, 1] or top >= 1, min_hits >= 1, penalty finite as a float32 and >= 0      VDET_EINVAL.
 *                                                                     A video whose records outgrow the scratch (an all-equal
 *                                                                     volume) takes the full-read passes: same results
 *   Seq-NMS                                (vdet_seq_nms, vdet_seq_nms_batch) 1 <= R <= 256 rows per (frame, class) (cut wider
 *                                          lists with vdet_nms_tracks' R), 1 <= max_seqs <= 4096, C*R*F, C*max_seqs*V and the
 *                                          link words C*F*R*ceil(R/32) below 2^31 - 16, at most 65535 videos, link_thres and
 *                                          nms_thres finite, min_score not NaN, rescore 0 or 1                          VDET_EINVAL.
 *                                                                     A video whose predecessor table ((F_v*Rp + F_v) int16,
 *                                                                     Rp = R rounded up to 64) outgrows 128 KiB of LDS keeps
 *                                                                     it in global scratch: same results
 *   Soft-NMS of the per-frame lists        (vdet_soft_nms_tracks, vdet_soft_nms_tracks_batch) the row of vdet_nms_tracks
 *                                          (top_still + T <= 1024, 1 <= R <= 1024, B <= 32767, C*R*F and C*T*F < 2^31 - 16, at
 *                                          most 65535 videos), and method 0 or 1, sigma finite and >= 1/64, thresh and
 *                                          min_score not NaN                                                     VDET_EINVAL; bad
 *                                                                     keep data, a zero union and R below a list's count as
 *                                                                     in vdet_nms_tracks.  One path for every size
 *   Box voting on the per-frame lists      (vdet_vote_nms_tracks, vdet_vote_nms_tracks_batch) the row of vdet_nms_tracks, and
 *                                          weights 0 or 1, vote_thresh not NaN                                   VDET_EINVAL; bad
 *                                                                     keep data, a zero union OF THE NMS and R below a list's
 *                                                                     count as in vdet_nms_tracks.  One path for every size
 *   NMS over whole tubelets: slots         (vdet_nms_tubelets, vdet_nms_tubelets_batch) 1 <= T <= 256 tubelet slots per class
 *                                          (the bit rows and the order of a class live in one wave's LDS), C*T*F < 2^31 - 16,
 *                                          at most 65535 videos, 0 .. 4 series                                  VDET_EINVAL
 *   NMS over whole tubelets: settings      thresh not NaN, min_shared >= 1, norm 0 .. 2 (union, shared, min), score_mode 0 .. 2
 *                                          (a score per slot [C,T], mean or max of a series [C,T,F])             VDET_EINVAL.
 *                                                                     Nothing is an error on the device: a box that gives no
 *                                                                     finite positive quotient contributes 0.  One path for
 *                                                                     every size
 */
#ifndef VDET_HIP_H
#define VDET_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vdet_ctx vdet_ctx;

typedef enum vdet_status {
    VDET_OK = 0,
    VDET_EINVAL = -1,    /* bad shape / argument  (python: ValueError) */
    VDET_ECAP = -2,      /* output capacity too small; nothing written past capacity (ValueError) */
    VDET_EHIP = -3,      /* HIP runtime failure (RuntimeError) */
    VDET_EDIVZERO = -4,  /* zero union where the reference raises ZeroDivisionError
                            (Cython cdivision=False, utils/nms.pyx:64,122,180) */
    VDET_ENOMEM = -5,
    VDET_EINDEX = -6,    /* where the reference raises IndexError (do_score_completion on a tubelet
                            without any valid score, vdet/tubelet_cls.py:293-295) */
    VDET_EAGAIN = -7     /* vdet_sync only, asynchronous mode (vdet_set_async): a suppression-graph build
                            ran out of scratch; the results since the last vdet_sync are invalid, the
                            scratch has been enlarged -- enqueue the same calls again (RuntimeError) */
} vdet_status;

/* ---- context ------------------------------------------------------------------------------- */

/* device < 0: use the calling thread's current HIP device. */
int vdet_create(vdet_ctx **out, int device);
int vdet_destroy(vdet_ctx *ctx);
/* Enqueue on an existing hipStream_t, used verbatim (e.g. torch's current stream; NULL = HIP's null
 * stream, which is torch's default stream). */
int vdet_set_stream(vdet_ctx *ctx, void *hip_stream);
/* Back to the context's own (non-blocking) stream, the default after vdet_create. */
int vdet_reset_stream(vdet_ctx *ctx);
/* Wait for the context's stream; return (and clear) the first latched device-side failure. */
int vdet_sync(vdet_ctx *ctx);
const char *vdet_last_error(vdet_ctx *ctx);
/* "vdet_hip <version> gfx950" */
const char *vdet_version(void);
/* Wall-clock (ms, HIP events on the context's stream) of the kernels enqueued since the events were
 * last read, summed by stage; used by bench.py for the roofline object.  out[16]: 0 iou_bits_sym
 * (K1s), 1 adj_build (K2), 2 sort (K3), 3 walk (K4), 4 temporal, 5 merge sort, 6 iou_bits general
 * (K1), 7 other, 8 transpose_keys, 9 track_pick, 10 track_link, 11 track_suppress,
 * 12 rescore_spatial, 13 rescore_series, 14-15 unused. */
int vdet_last_timing_ms(vdet_ctx *ctx, float *out16);
/* Number of timed launches per stage behind the sums of vdet_last_timing_ms (call it first). */
int vdet_last_launches(vdet_ctx *ctx, int *out16);
/* Opt-in reuse of the per-video preparation between d_* calls: with the cache enabled,
 * vdet_nms_volume / vdet_track_volume skip the suppression-graph build (same d_boxes pointer, shape
 * and threshold) and the per-(frame,class) sort (same d_scores pointer/layout) of the previous call.
 * The CALLER promises the buffers' contents did not change; vdet_invalidate() drops the cache (call
 * it whenever a buffer was rewritten in place).  Default: disabled. */
int vdet_set_cache(vdet_ctx *ctx, int enable);
int vdet_invalidate(vdet_ctx *ctx);
/* Asynchronous video step (default: disabled).  When enabled, the d_* volume entry points
 * (vdet_nms_volume, vdet_track_volume, vdet_nms_track_volume, vdet_rescore_tracks, vdet_volume_pass)
 * never wait for the device once the context has built one suppression graph: the per-geometry launch
 * tables stay resident, the device status words stay latched until vdet_sync, and the scratch for the
 * adjacency lists is sized from the largest graph seen so far (+50 %).  A graph that still outgrows
 * it makes the next vdet_sync return VDET_EAGAIN (nothing is written out of bounds). */
int vdet_set_async(vdet_ctx *ctx, int enable);
/* Introspection: what = 0 -> 1 if the per-(frame,class) sort uses the returning-LDS-atomic rank
 * (selected by a hardware self-test at vdet_create), 0 if it uses the ballot match;
 * what = 1 -> number of compute units;
 * what = 2 -> 1 if every frame of the last SYNCHRONOUS suppression-graph build was "regular" (finite
 * boxes, positive width / height / area); 0 after an asynchronous build (not known on the host);
 * what = 3 -> 1 if the 64x64 in-wave bit transpose passed its self-test at vdet_create;
 * what = 4 / 5 -> link steps of the last tracking call that were served by the link memo / that scanned their
 * frame (synchronises the stream); 6 / 7 -> the same for the memo warm-up launch;
 * what = 8 -> number of host waits (hipStreamSynchronize) this context has made so far: the asynchronous video
 * step (vdet_set_async) adds none between the entry and the return of the volume entry points;
 * what = 9 -> (frame, class) columns of the last volume sort that the equalised counting sort handed to the LSD
 * radix kernel (tied / quantised / thresholded columns; synchronises the stream), -1 if that sort did not use it;
 * what = 10 -> number of times the device TCN's parameters were uploaded (a call with the resident net uploads nothing);
 * what = 11 -> number of times the per-video table of vdet_top_anchors (batch form), vdet_track_from_anchors_batch and
 * vdet_anchor_propagate_tracks_batch was staged (calls with the same frame offsets stage it once);
 * what = 12 -> which kernel the last vdet_volume_pass[_batch] launched: 4 the current fused kernel, 2 the lean one
 * (vdet_set_vpass), 0 the separate temporal kernels; 104: the current kernel held to one block per compute unit.
 * what = 13 -> full reads of the volume the last vdet_context_classes needed, the most of any of its videos: 2, 3 (the records
 * fit only below the second digit) or 4 (they never fit, or VDET_CTX_RECORDS=0); 0 when no video had a candidate; -1 before
 * the first call (synchronises the stream).
 * what = 14 -> where the last vdet_seq_nms[_batch] kept the predecessor table: 1 in LDS, 2 in global scratch (the longest video's
 * table outgrew the LDS budget, or VDET_SEQNMS_LDS=0); -1 before the first call.
 * what = 15 -> 1 if the last suppression-graph build took the direct lists.
 * what = 16 -> (frame, class) columns of the last volume sort that the counting sort ordered with the key -> bin map INHERITED
 * from the column its workgroup sorted before (no histogram of their own; the order does not depend on the map);
 * what = 17 -> columns whose inherited map overflowed a bin and that were sorted AGAIN with their own map (they do not go to the
 * LSD kernel and are not counted by 16).  Both synchronise the stream; -1 if that sort did not use the counting sort.
 * what = 18 -> (frame, class) lists of the last volume walk that entered the WIDE filter of the packed walk (four chunks of 64
 * candidates tested per pass once a pass queued fewer than 12; the keep lists do not depend on it);
 * what = 19 -> wide passes of that walk that wanted more than 64 candidates and were queued chunk by chunk instead.  Both
 * synchronise the stream; -1 if the last walk could not take the wide filter (VDET_WALK_WIDE=0, no regular frame).
 *
 * Environment switches, read once by vdet_create (diagnostics: each FORCES a fallback path the library takes anyway on some
 * inputs or devices, with identical results; none selects a tuning variant -- the one switch that does, VDET_VPASS_FORM,
 * is described with vdet_set_vpass):
 *   VDET_FORCE_GENERAL=1  the all-pairs predicate kernel + one-survivor walk on every frame (what irregular frames take)
 *   VDET_NO_INDEX=1       no x-sorted proposal index (what frames too large for it take)
 *   VDET_NO_LAZY=1        eager track_det_nms of every crossed list (what irregular frames take)
 *   VDET_NO_FUSED=1       h_* calls of <= 640 rows through the general kernel chain (what larger inputs take)
 *   VDET_BINSORT=0        the LSD radix sort for every column (what tied / thresholded columns take)
 *   VDET_BINSORT_INHERIT=0  every column of the counting sort builds its own key -> bin map (what a column takes whose
 *                         predecessor's map does not fit its scores)
 *   VDET_BINSORT_GRID=n   at most n workgroups for the counting sort (1: one workgroup sorts the columns in order)
 *   VDET_WALK_WIDE=0      the packed walk filters every list 64 candidates per pass to its end (what a list takes until a pass
 *                         queues fewer than 12 candidates); VDET_WALK_WIDE_NSW=n (1..63) moves that switch point
 *   VDET_SMALL_LISTS=0    frames of <= 384 boxes through the large-list sort and walk
 *   VDET_DIRECT_LISTS=0   the suppression graph of regular frames of > 384 boxes through the bit matrix (what a context takes for
 *                         good once a row had more neighbours than a direct list slot holds); VDET_DIRECT_CAP=n entries per slot
 *   VDET_ADJ_ROWS=0       (bit-matrix path) the lane-per-row adjacency kernel on every frame (what irregular / small frames take)
 *   VDET_TCN_TILED=1      device TCN: every series cut into the smallest tiles, 16 positions or the net's halo (what long series
 *                         and wide nets take)
 *   VDET_TCN_GLOBAL=1     device TCN: the activations in global memory (what nets too wide for the LDS budget take)
 *   VDET_CTX_RECORDS=0    vdet_context_classes: no record scratch, every digit round and the per-class count by a full read of
 *                         the volume (what a video takes whose records outgrow the scratch: an all-equal volume)
 *   VDET_SEQNMS_LDS=0     vdet_seq_nms: the predecessor table of the best-path pass in global scratch (what long videos take)
 *   VDET_ATOMIC_RANK=0 / VDET_WAVE_TRANSPOSE=0   the variants selected when the start-up hardware probes fail
 *   VDET_BITS_BUDGET_MB=n bytes of bit-matrix scratch per graph-build batch (default 1024) */
int vdet_query(vdet_ctx *ctx, int what);
/* Per-stage HIP-event timing: 0 off (default), 1 on (events of the most recent call), 2 on and
 * accumulating over calls until vdet_last_timing_ms reads them. */
int vdet_set_timing(vdet_ctx *ctx, int enable);

/* ---- utils/cython_nms replacements (host buffers, synchronous) ------------------------------- */

/*
 * nms      (utils/nms.pyx:17-68)   ncols == 5, rows (x1,y1,x2,y2,score)
 * vid_nms  (utils/nms.pyx:71-125)  ncols == 6, rows (frame,x1,y1,x2,y2,score); detections on
 *                                  different frames (float32 equality, :111) never suppress.
 * h_dets: float32, n rows, row stride `ld` elements (>= ncols).  thresh is the reference's boxed
 * python float: suppression iff (double)ovr_f32 >= thresh.  h_order: NULL, or the n indices the
 * reference's argsort()[::-1] produced (tie reproduction).  h_keep: capacity n; receives indices
 * in descending score order; *n_keep their count.  VDET_EDIVZERO mirrors ZeroDivisionError.
 */
int vdet_nms_f32(vdet_ctx *ctx, const float *h_dets, int64_t n, int64_t ld, int ncols,
                 double thresh, const int64_t *h_order, int64_t *h_keep, int64_t *n_keep);

/*
 * track_det_nms (utils/nms.pyx:128-189): h_tracks t rows (frame,x1,y1,x2,y2) stride ldt;
 * h_dets m rows (frame,x1,y1,x2,y2,score) stride ldd.  Round 1: a det is dropped when it overlaps
 * (IoU >= thresh, det as the "i" box) a same-frame track; round 2: vid_nms among the survivors.
 * h_keep (capacity m): indices into dets, descending score.
 */
int vdet_track_det_nms_f32(vdet_ctx *ctx, const float *h_tracks, int64_t t, int64_t ldt,
                           const float *h_dets, int64_t m, int64_t ldd, double thresh,
                           int64_t *h_keep, int64_t *n_keep);

/*
 * The reference's per-tracked-box pattern (vdet/track.py:236-250 and :170-184: one track_det_nms call per box of every new
 * tracklet, each against the still-kept detections of that box's frame) as ONE call: K independent problems, problem k =
 * track_det_nms(h_tracks[h_toff[k] .. h_toff[k+1]), h_dets[h_off[k] .. h_off[k+1]), thresh).  h_toff == NULL: exactly one
 * track row per problem (row k).  h_keep (capacity h_off[K]): problem k's kept indices -- positions inside ITS rows,
 * descending score -- start at h_keep[h_off[k]]; h_nkeep[k] their count.  Problems of <= 640 rows run as one launch of K
 * workgroups and one host wait; otherwise the problems are taken one after the other.  The caller guarantees the problems
 * are independent (the boxes of one tracklet sit on different frames); a frame that repeats belongs in the next call.
 */
int vdet_track_det_nms_batch(vdet_ctx *ctx, const float *h_tracks, const int64_t *h_toff, int64_t ldt,
                             const float *h_dets, const int64_t *h_off, int64_t K, int64_t ldd, double thresh,
                             int64_t *h_keep, int64_t *h_nkeep);

/* iou (utils/common.py:451-468): float64 IoU matrix out[n1,n2] of boxes1[n1,4] x boxes2[n2,4]. */
int vdet_iou_f64(vdet_ctx *ctx, const double *h_boxes1, int64_t n1, const double *h_boxes2,
                 int64_t n2, double *h_out);

/*
 * svm_scores (vdet/image_det.py:109-114), the path's one dense contraction:
 *     out[n, m] = feat[n, k] . W[k, m] + B[m]          (B may be NULL)
 * as a hand-written MFMA kernel (v_mfma_f64_16x16x4_f64 / v_mfma_f32_16x16x4_f32): the reference computes it in
 * numpy's result dtype -- float64 with its .mat SVM models, float32 when features and W are float32.  The feature
 * scaling `features * (20 / feat_norm_mean)` stays with the caller (it is rounded in the features' dtype first, :112).
 * Row-major host buffers; per output element the products are accumulated in ascending k, one fma each.
 */
int vdet_svm_scores_f64(vdet_ctx *ctx, const double *h_feat, int64_t n, int64_t k, const double *h_W,
                        const double *h_B, int64_t m, double *h_out);
int vdet_svm_scores_f32(vdet_ctx *ctx, const float *h_feat, int64_t n, int64_t k, const float *h_W,
                        const float *h_B, int64_t m, float *h_out);

/* ---- tubelet re-scoring cores (host buffers, synchronous, float64 like the reference) --------- */

/*
 * Spatial max-pooling core of raw_dets_spatial_max_pooling / dets_spatial_max_pooling
 * (vdet/tubelet_cls.py:514-532, :327-347).  T tubelet boxes h_tub_boxes[T,4]; box t lives on frame
 * slot h_tub_group[t] whose detections are rows [h_group_off[g], h_group_off[g+1]) of
 * h_det_boxes[M,4] / h_det_scores[M] (the class column).  Among the detections with
 * iou > thres (strict, float64, utils/common.py:451-468) the first arg-max of the score (np.argmax:
 * first occurrence, NaN wins): h_out_idx[t] = its index within the frame (-1: none overlaps),
 * h_out_score[t] = its score (-1e5 when none, :529).
 */
int vdet_spatial_maxpool_f64(vdet_ctx *ctx, const double *h_tub_boxes, const int32_t *h_tub_group, int64_t T,
                             const double *h_det_boxes, const double *h_det_scores,
                             const int64_t *h_group_off, int64_t G, double thres, int64_t *h_out_idx,
                             double *h_out_score);

/*
 * do_score_completion (vdet/tubelet_cls.py:284-303) on T ragged series h_vals[h_off[t]..h_off[t+1]),
 * in place.  VDET_EINDEX where the reference raises IndexError (whole series <= -10).
 */
int vdet_series_completion_f64(vdet_ctx *ctx, double *h_vals, const int64_t *h_off, int64_t T);

/* score_proto_temporal_maxpool core (vdet/tubelet_cls.py:399-412) on T ragged float64 series. */
int vdet_series_maxpool_f64(vdet_ctx *ctx, const double *h_in, double *h_out, const int64_t *h_off,
                            int64_t T, int window, double pad);

/*
 * score_proto_interpolation core (vdet/tubelet_cls.py:453-487; scipy interp1d linear ==
 * numpy.interp, plus extrap1d :416-428).  Per tubelet t: knots h_x[h_koff[t]..h_koff[t+1])
 * (ascending, >= 2), K fields stored field-major h_y[h_koff[t]*K + f*L + k]; queries
 * h_q[h_qoff[t]..h_qoff[t+1]); results h_out[h_qoff[t]*K + f*Lq + n].
 */
int vdet_series_interp_f64(vdet_ctx *ctx, const double *h_x, const double *h_y, const int64_t *h_koff,
                           const double *h_q, const int64_t *h_qoff, int64_t T, int K, double *h_out);

/*
 * Per-class threshold + top-k of ONE frame (vdet/video_det.py:89-99).  h_scores [B, ld] float32
 * (is_f64 = 0) or float64 (1); class columns col0 .. col0+ncls-1.  Per class: inds = rows with
 * score > thresh; if more than k: the k best by argsort(-score) (stable), in that order; else all
 * of them in ascending row order.  h_idx [ncls, k] int32, h_cnt [ncls] int32.
 */
int vdet_threshold_topk(vdet_ctx *ctx, const void *h_scores, int is_f64, int64_t B, int64_t ld, int col0,
                        int ncls, double thresh, int k, int32_t *h_idx, int32_t *h_cnt);

/*
 * One temporal-convolution layer of the tubelet TCN (the build's stand-in for the external Caffe
 * net that score_conv_cls feeds, vdet/tubelet_cls.py:15-51; parity unpinned):
 *   out[co,l] = act(b[co] + sum_ci sum_k w[co,ci,k] * in[ci, l+k-K/2]), zero padded, f32,
 * accumulated ci-outer / k-inner without contraction.  h_in [Cin,L], h_w [Cout,Cin,K], h_b [Cout],
 * h_out [Cout,L]; K odd.  act: 0 none, 1 ReLU, 2 softmax over the Cout channels (applied after the
 * affine part, like Caffe's SoftmaxLayer).
 */
int vdet_conv1d_f32(vdet_ctx *ctx, const float *h_in, int Cin, int L, const float *h_w, const float *h_b,
                    int Cout, int K, int act, float *h_out);

/* ---- device-resident array forms (asynchronous; see vdet_sync) ------------------------------- */

#define VDET_LAYOUT_FBC 0 /* scores [F,B,C], class innermost (zs[B,C], utils/protocol.py:538) */
#define VDET_LAYOUT_FCB 1 /* scores [F,C,B] */

/*
 * Per-(frame,class) greedy NMS over a whole video: apply_image_nms (vdet/image_det.py:117-123)
 * for every frame and class of fast_rcnn_det_vid's per-class loop (vdet/video_det.py:89-99),
 * == vid_nms (utils/nms.pyx:71-125) of each class decomposed per frame.
 *   d_boxes  [F,B,4] f32    d_scores [F,B,C] or [F,C,B] f32
 *   use_score_thresh != 0: only boxes with score > score_thresh are candidates (video_det.py:90)
 *   d_keep_idx [F,C,cap] int32: kept box indices (0..B-1), descending score; entries >= count
 *                               are left untouched.   d_keep_cnt [F,C] int32.
 *   A (frame,class) with more than cap survivors latches VDET_ECAP (its count is still written).
 * Limits: see the table at the top of this file (B <= ~18000).
 */
int vdet_nms_volume(vdet_ctx *ctx, const float *d_boxes, const float *d_scores, int layout,
                    int64_t F, int64_t B, int64_t C, double thresh, int use_score_thresh,
                    float score_thresh, int32_t *d_keep_idx, int32_t *d_keep_cnt, int64_t cap);

/*
 * vdet_nms_volume preceded, on the device, by the per-class candidate selection of
 * fast_rcnn_det_vid (vdet/video_det.py:89-99): per (frame, class) the candidates are the boxes with
 * score > score_thresh (use_score_thresh; float32 compare like numpy's), and when more than `topk`
 * (> 0; the reference's max_per_image = 100) remain only the topk best -- argsort(-scores)[:topk],
 * i.e. ties at the cut go to the LOWEST indices -- enter the NMS.  The reference's pipeline order
 * (threshold -> top-k -> apply_image_nms, vdet/image_det.py:117-123) without the scores ever leaving
 * HBM.  topk == 0: no cut (== vdet_nms_volume).
 */
int vdet_nms_volume_topk(vdet_ctx *ctx, const float *d_boxes, const float *d_scores, int layout,
                         int64_t F, int64_t B, int64_t C, double thresh, int use_score_thresh,
                         float score_thresh, int topk, int32_t *d_keep_idx, int32_t *d_keep_cnt,
                         int64_t cap);

/*
 * The Fast R-CNN per-class flow on the device: fast_rcnn_det_vid's per-class loop (vdet/video_det.py:89-99) followed by
 * apply_image_nms (vdet/image_det.py:117-123 -> utils/nms.pyx:17-68) for every frame and class, where -- unlike the
 * vdet_nms_volume family -- every class suppresses ITS OWN regressed boxes (boxes[inds, 4j:4j+4], video_det.py:92).
 *   d_boxes  [F,B,K,4] f32 (== the reference's [B, 4K] box array per frame), 16-byte aligned
 *   d_scores [F,B,K]   f32;  classes j < class0 are skipped (class0 = 1: the background column)
 *   candidates of (frame, j): score > score_thresh (use_score_thresh; float32 compare); more than topk (the
 *   reference's max_per_image, <= 128) -> the topk best, argsort(-score)[:topk] (ties at the cut: lowest indices)
 *   d_dets    [F,K,topk,5] f32 or NULL: the rows (x1,y1,x2,y2,score) in the REFERENCE's row order -- ascending box
 *             index, or descending score when the cut applied (video_det.py:93-97)
 *   d_sel_idx [F,K,topk] int32 or NULL: the box index of every row;  d_det_cnt [F,K] rows per (frame, class)
 *   d_keep    [F,K,topk] int32: the kept ROW positions in descending score order (apply_image_nms's list),
 *   d_keep_cnt [F,K].  Entries behind the counts are left untouched.
 * A zero-union pair that the reference would evaluate latches VDET_EDIVZERO (reported by vdet_sync).
 */
int vdet_det_nms_volume(vdet_ctx *ctx, const float *d_boxes, const float *d_scores, int64_t F, int64_t B, int64_t K,
                        int class0, int use_score_thresh, float score_thresh, int topk, double nms_thresh,
                        float *d_dets, int32_t *d_sel_idx, int32_t *d_det_cnt, int32_t *d_keep, int32_t *d_keep_cnt);

/*
 * The Fast R-CNN box decode on the device: image_det.bbox_transform_inv followed by clip_boxes, per box and class.
 * THE rule, bit for bit, is tests/decode_spec.py.  With the roi (x1,y1,x2,y2) widened exactly to f64 and the class's deltas
 * (dx,dy,dw,dh) f32 widened exactly:
 *     w = (x2 - x1) + 1e-14,  cx = x1 + 0.5*w,  pcx = dx*w + cx,  pw = E(dw)*w,  X1 = pcx - 0.5*pw,  X2 = pcx + 0.5*pw
 * (y alike); every product and sum is one f64 operation (no fused multiply-add), then x is clipped to [0, W-1] and y to
 * [0, H-1] -- clip(v, hi) = NaN if v is NaN, hi if v > hi, v if v > 0, else +0.0: numpy's maximum(minimum(v, hi), 0), a NaN
 * stays and -0.0 becomes +0.0 -- and rounded ONCE to f32.  E is an exponential as a fixed sequence of f64 operations
 * (k = rint(x*log2e), r = (x - k*ln2_hi) - k*ln2_lo, a degree-13 Horner polynomial with coefficients 1/n!, ldexp): within
 * 2 units in the last place of exp; NaN -> NaN, x > 709 -> +inf, x < -708 -> +0.0.  dw is not clamped.  A roi or delta that
 * is not finite gives NaN or clipped coordinates, never an error.
 *   d_rois   [N,4] f32 or f64 (rois_f64), d_deltas [N,K,4] f32 (== the head's [N, 4K] rows), d_boxes [N,K,4] f32; all three
 *   16-byte aligned (VDET_EINVAL otherwise).  H, W >= 1.  N*K up to 2^40; N = 0 or K = 0 is legal.  One launch.
 */
int vdet_decode_boxes(vdet_ctx *ctx, const void *d_rois, int rois_f64, const float *d_deltas, int64_t N, int64_t K, int64_t H,
                      int64_t W, float *d_boxes);

/*
 * vdet_det_nms_volume reading the head's output instead of decoded boxes: d_rois [F,B,4] f32 or f64 (rois_f64), d_deltas
 * [F,B,K,4] f32, both 16-byte aligned (VDET_EINVAL otherwise), H, W >= 1.  The selection is the same one, on the scores; the
 * wave of a (frame, class) then decodes its <= topk candidates at the gather (vdet_decode_boxes' rule) and goes on as
 * vdet_det_nms_volume does.  No [F,B,K,4] tensor exists at any point.  Every output, and every status vdet_sync reports, is
 * bit for bit that of vdet_det_nms_volume on vdet_decode_boxes' output.  Limits and the remaining arguments are
 * vdet_det_nms_volume's.
 */
int vdet_det_nms_volume_deltas(vdet_ctx *ctx, const void *d_rois, int rois_f64, const float *d_scores, const float *d_deltas,
                               int64_t F, int64_t B, int64_t K, int64_t H, int64_t W, int class0, int use_score_thresh,
                               float score_thresh, int topk, double nms_thresh, float *d_dets, int32_t *d_sel_idx,
                               int32_t *d_det_cnt, int32_t *d_keep, int32_t *d_keep_cnt);

/*
 * The tubelet side of the decode (what fast_rcnn_cls computes per tubelet box): for the compact row n < count of
 * vdet_tubelet_rois with d_slot[n] = (c,t,f) and col = d_cols[c] (d_cols NULL: c + 1, column 0 being the background)
 *     d_det[c,t,f]    = (double)d_scores[n, col]
 *     d_tboxes[c,t,f] = decode(d_tracks[c,t,f,0:4], d_deltas[n, 4*col : 4*col+4])          (vdet_decode_boxes' rule)
 *   d_scores [N,K] f32, d_deltas [N,K,4] f32 (16-byte aligned), d_tracks [C,T,F,ld] f32 or f64 (tracks_f64), ld >= 4,
 *   d_slot [N,3] int32, d_count [1] int32 or NULL (all N rows; rows behind the count are not read), d_cols [C] int32 or NULL,
 *   d_det [C,T,F] f64, d_tboxes [C,T,F,4] f32 (16-byte aligned).  Slots that no row names are left untouched.
 * A slot outside (C,T,F) or a column outside 0..K-1 latches VDET_EINVAL (reported by vdet_sync); that row is skipped.
 * C, T, F >= 1, C*T*F < 2^31 - 16.  One launch, one thread per row.
 */
int vdet_tubelet_dets(vdet_ctx *ctx, const float *d_scores, const float *d_deltas, int64_t N, int64_t K, const void *d_tracks,
                      int tracks_f64, int ld, const int32_t *d_slot, const int32_t *d_count, int64_t C, int T, int64_t F,
                      const int32_t *d_cols, int64_t H, int64_t W, double *d_det, float *d_tboxes);

/*
 * vdet_det_nms_volume[_deltas]' outputs in the rank layout vdet_nms_tracks writes, C = K - class0 classes, R = topk ranks:
 *   d_tracks [C,R,F,5] f32: the kept rows of (frame f, class class0 + c) in keep order (descending score),
 *   d_score [C,R,F] f64 the row's score, d_src [C,R,F] int32 the row's box index (d_sel_idx), d_cnt [C,F] = d_keep_cnt,
 *   d_ntracks [C] = the maximum of d_cnt over the frames (an integer atomic maximum).  Behind the counts: NaN, INT32_MIN.
 * d_dets must be given ([F,K,topk,5]).  A keep count beyond topk is read as topk, a kept row outside 0..topk-1 as a row behind
 * the count.  F, K >= 1, 0 <= class0 < K, 1 <= topk <= 128, K*topk*F < 2^31 - 16.  One launch (and a memset of d_ntracks).
 */
int vdet_dets_as_tracks(vdet_ctx *ctx, const float *d_dets, const int32_t *d_sel_idx, const int32_t *d_keep,
                        const int32_t *d_keep_cnt, int64_t F, int64_t K, int topk, int class0, float *d_tracks, double *d_score,
                        int32_t *d_src, int32_t *d_cnt, int32_t *d_ntracks);

/*
 * vdet_nms_volume with the CALLER's order instead of the build's: d_order [F,C,B] uint16 lists every (frame, class)
 * column's candidates in the order the greedy loop of utils/nms.pyx:26-66 is to visit them (the first d_ncand[f,c]
 * entries; the rest is ignored), e.g. vdet_argsort_volume's lists with ties rearranged the way a particular machine's
 * unstable `scores.argsort()[::-1]` (utils/nms.pyx:25) left them -- the volume-scale form of vdet_nms_f32's h_order.
 * An entry must be a box index < B and appear once per list.
 */
int vdet_nms_volume_ordered(vdet_ctx *ctx, const float *d_boxes, const uint16_t *d_order, const int32_t *d_ncand,
                            int64_t F, int64_t B, int64_t C, double thresh, int32_t *d_keep_idx,
                            int32_t *d_keep_cnt, int64_t cap);

/*
 * The proposal layer of a region proposal network on the device (the boxes of the Faster R-CNN route): anchors, decode, clip,
 * size filter, top-N, NMS, top-N, for F frames of one image size.  THE rule, bit for bit, is tests/rpn_spec.py; it restates
 * the public py-faster-rcnn proposal layer, which was not at hand (parity with that code's f32 host arithmetic is unpinned).
 *   d_scores   f32, frame f / anchor a / cell (h,w) at d_scores[f*score_frame_stride + (a*Hf + h)*Wf + w]: the foreground half
 *              cls[:, A:] of a contiguous [F,2A,Hf,Wf] output goes in with a stride of 2*A*Hf*Wf and no copy.  Logits or
 *              probabilities: only the ranking is used.
 *   d_deltas   f32 [F,4A,Hf,Wf] contiguous, channel 4a+k component k of anchor a;  d_anchors f64 [A,4] (on the device).
 * The candidate of flat index n = (h*Wf + w)*A + a is the anchor d_anchors[a] + (w,h,w,h)*stride (f64) decoded by
 * vdet_decode_boxes' rule with the width term w = (x2 - x1) + offset (1.0: the RPN's; 1e-14: vdet_decode_boxes') and, with
 * use_dw_max, a dw / dh GREATER than dw_max replaced by dw_max (NaN stays), clipped to (H, W), rounded once to f32.  It is valid
 * when its score is not NaN and (X2 - X1) + 1 >= min_size and (Y2 - Y1) + 1 >= min_size on the f32 box, evaluated in f64.
 * Valid candidates are ordered by descending score, equal scores (-0.0 == +0.0) by DESCENDING n; the first pre_nms_top_n are
 * kept, greedy NMS at nms_thresh (vdet_nms_volume_ordered's arithmetic, one list per frame) runs over them in that order and
 * the first post_nms_top_n survivors are the proposals; more survivors are no error.
 *   d_rois [F,post,4] f32 (16-byte aligned), d_out_scores [F,post] f32, d_index [F,post] int32 (the flat index n), d_count [F]
 *   int32; behind the count: NaN, NaN, -1 -- written by this call, the buffers need no initialisation.
 *   d_cand_index [F,pre] int32 (-1 behind the count) / d_cand_cnt [F] int32: the candidates in order, or NULL.
 * Three launches of its own (decode, select, gather) around those of vdet_nms_volume_ordered on [F,pre,4] boxes with one list per
 * frame; scratch (a key and a box per anchor, the candidates, the keep list) is the context's.
 * No host wait on a context set asynchronous (vdet_set_async) once the NMS's pool size is known, as for vdet_nms_volume.
 * A frame with fewer than pre_nms_top_n candidates pads its NMS list with NaN boxes and takes the general predicate kernel.
 * The resident suppression graph of the prep cache is dropped by this call.
 */
int vdet_rpn_proposals(vdet_ctx *ctx, const float *d_scores, int64_t score_frame_stride, const float *d_deltas,
                       const double *d_anchors, int64_t F, int64_t A, int64_t Hf, int64_t Wf, int64_t H, int64_t W, int64_t stride,
                       int64_t pre_nms_top_n, int64_t post_nms_top_n, double nms_thresh, double min_size, double offset,
                       int use_dw_max, double dw_max, float *d_rois, float *d_out_scores, int32_t *d_index, int32_t *d_count,
                       int32_t *d_cand_index, int32_t *d_cand_cnt);

/*
 * Batched small videos (BASELINE configs[0] / [4] shapes: hundreds of frames x <= 300 boxes x 30 classes -- a single
 * such video is launch-bound).  The frames of V videos are concatenated along F; h_frame_off [V+1] (host, starts at 0,
 * strictly increasing) gives every video its frame range.  What does not look across frames -- the suppression graph,
 * the per-(frame, class) sorts and NMS walks (vdet/video_det.py:79-106 over utils/nms.pyx) -- runs ONCE for the whole
 * batch; tracking and re-scoring (vdet/track.py:189-252, vdet/tubelet_cls.py:493-535, :284-303, :386-414) run per
 * video on its frame range with the video as a grid dimension (one launch per stage for ALL videos).  Results are what vdet_nms_track_volume + vdet_rescore_tracks return
 * for each video on its own, laid out video after video:
 *   d_tracks [sum_v C*T*F_v*5] (video v at C*T*5*h_frame_off[v]), d_anchors [V,C,T,3], d_ntracks [V,C],
 *   d_keep_idx [F,C,cap] / d_keep_cnt [F,C] over the concatenated frames (d_keep_cnt null: no NMS output),
 *   d_det_score / d_pooled [sum_v C*T*F_v] f64, d_boxes_out [sum_v C*T*F_v*4] (d_pooled null: no re-scoring).
 */
int vdet_video_batch(vdet_ctx *ctx, const float *d_boxes, const float *d_scores, const int64_t *h_frame_off,
                     int64_t V, int64_t B, int64_t C, double nms_thres, double thres, int max_tracks,
                     double link_thres, int max_frames, float *d_tracks, float *d_anchors, int32_t *d_ntracks,
                     int64_t cap, int32_t *d_keep_idx, int32_t *d_keep_cnt, double overlap_thres, int window,
                     double *d_det_score, double *d_pooled, float *d_boxes_out);

/*
 * vdet_volume_pass over V concatenated videos: a temporal window stops at its video's first / last frame (frames of
 * another video count as padding, like frames outside [0, F) of a single video).  Same outputs and layouts.
 */
int vdet_volume_pass_batch(vdet_ctx *ctx, const float *d_scores, const int64_t *h_frame_off, int64_t V, int64_t B,
                           int64_t C, int window, float pad_max, const float *h_taps, float bias, float pad_conv,
                           float *d_out_max, float *d_out_conv, int use_score_thresh, float score_thresh);

/*
 * Descending argsort of every (frame, class) score column of a volume: the order utils/nms.pyx:25
 * (`scores.argsort()[::-1]`) and vdet/video_det.py:93 (`argsort(-cls_scores)`) walk, with the build's
 * deterministic tie rule (equal scores by DESCENDING index, -0.0 == +0.0, NaN first).
 *   d_scores [F,B,C] or [F,C,B] f32 (layout)   use_score_thresh != 0: boxes with score <= score_thresh are
 *   no candidates and go to the tail.   d_order [F,C,B] uint16: box indices;   d_ncand [F,C] int32: candidates.
 * The same lists vdet_nms_volume / vdet_track_volume build internally (equalised counting sort, LSD radix
 * sort for tied / thresholded columns).  B <= ~18000.
 */
int vdet_argsort_volume(vdet_ctx *ctx, const float *d_scores, int layout, int64_t F, int64_t B, int64_t C,
                        int use_score_thresh, float score_thresh, uint16_t *d_order, int32_t *d_ncand);

/*
 * Centred sliding temporal max over series laid out [F,S] (series s = in[f*S+s]); the array form
 * of score_proto_temporal_maxpool (vdet/tubelet_cls.py:386-414): out[f] = max(in[f-h..f+h]),
 * out-of-range samples = pad (-1e5 in the reference, :402); NaN propagates (np.max).  window must
 * be odd (else VDET_EINVAL, the reference's ValueError :389-390).  d_in != d_out.
 * For a score volume [F,B,C] pass S = B*C.
 */
int vdet_temporal_maxpool_f32(vdet_ctx *ctx, const float *d_in, float *d_out, int64_t F, int64_t S,
                              int window, float pad);

/*
 * Single-channel temporal convolution over [F,S] series: out[f] = bias + sum_k taps[k] *
 * in[f+k-K/2] (out-of-range = pad), accumulated left to right in f32, no FMA contraction.
 * Stands in for the external Caffe TCN of score_conv_cls (vdet/tubelet_cls.py:15-51), whose
 * prototxt/weights are not part of the reference tree (parity unpinned).
 * h_taps: K (odd, <= 31) host floats.
 */
int vdet_temporal_conv_f32(vdet_ctx *ctx, const float *d_in, float *d_out, int64_t F, int64_t S,
                           const float *h_taps, int K, float bias, float pad);

/* Both temporal operators of one volume in one pass (the volume is read once): d_out_max as
 * vdet_temporal_maxpool_f32(window, pad_max), d_out_conv as vdet_temporal_conv_f32(h_taps[window],
 * bias, pad_conv).  Bit-identical to the two separate calls. */
int vdet_temporal_maxpool_conv_f32(vdet_ctx *ctx, const float *d_in, float *d_out_max, float *d_out_conv, int64_t F,
                                   int64_t S, int window, float pad_max, const float *h_taps, float bias, float pad_conv);

/*
 * The one pass over a class-innermost score volume d_scores [F,B,C] (zs[B,C] per frame,
 * utils/protocol.py:538): every score is read ONCE and produces
 *   d_out_max  [F,B,C]  = vdet_temporal_maxpool_f32(window, pad_max)        (vdet/tubelet_cls.py:386-414)
 *   d_out_conv [F,B,C]  = vdet_temporal_conv_f32(h_taps[window], bias, pad_conv); h_taps NULL: none
 *   and, inside the context, the class-major sort keys of all F*C per-(frame, class) problems
 *   (score > score_thresh candidates only when use_score_thresh), which the next
 *   vdet_nms_volume[_topk] (layout FBC) / vdet_track_volume / vdet_nms_track_volume call on the SAME
 *   d_scores, shape and score threshold then uses instead of reading the volume again -- under the
 *   vdet_set_cache contract (cache enabled, buffers unchanged in between; vdet_invalidate drops them).
 * Bit-identical to the separate calls.  Shapes the fused kernel does not cover (C % 4 != 0, window
 * other than 3 / 5, unaligned pointers) run the separate temporal kernels and leave no keys.
 */
int vdet_volume_pass(vdet_ctx *ctx, const float *d_scores, int64_t F, int64_t B, int64_t C, int window,
                     float pad_max, const float *h_taps, float bias, float pad_conv, float *d_out_max,
                     float *d_out_conv, int use_score_thresh, float score_thresh);

/*
 * Which form of the fused kernel vdet_volume_pass[_batch] launches.  Every form computes the same outputs bit for bit; they
 * differ in what a resident block takes from a compute unit (DESIGN.md section 7 has the registers and the LDS of each).
 *   VDET_VPASS_AUTO       the host chooses: VDET_VPASS_ONE_PER_CU for a context that runs asynchronously with the cache on
 *                         (vdet_set_async + vdet_set_cache: the multi-video pipeline, whose streams share the chip), window 3
 *                         and the 512-thread tiling (C > 128); VDET_VPASS_CURRENT otherwise
 *   VDET_VPASS_CURRENT    4 items per thread, one block per (tile, frame chunk)
 *   VDET_VPASS_LEAN       (measurements only: it bought nothing) 2 items per thread, half the tile, 2 blocks per compute unit
 *                         that stride over the work; window 3 only, and a class count
 *                         whose 16-box tile does not fit 512 x 2 items (C > 256) takes the current form
 *   VDET_VPASS_ONE_PER_CU the current form, its dynamic LDS padded so that one block is resident per compute unit: alone the
 *                         HBM-bound pass is as fast as with two, and kernels of other streams find room next to it
 * fchunk > 0 sets the frames per chunk (0: the host's formula; a value that would make more than 65 535 chunks is raised
 * until they fit); tests force chunk seams into short videos with it.
 * The environment variables VDET_VPASS_FORM=<number> and VDET_VPASS_FCHUNK=<frames>, read once by vdet_create, set the
 * same two values for every context of the process.
 */
#define VDET_VPASS_AUTO 0
#define VDET_VPASS_CURRENT 1
#define VDET_VPASS_LEAN 2
#define VDET_VPASS_ONE_PER_CU 3
int vdet_set_vpass(vdet_ctx *ctx, int form, int fchunk);

/*
 * Greedy tubelet generation for every class of a score volume, device-resident: the array form of
 * greedily_track_from_raw_dets (vdet/track.py:189-252) with the built-in IoU-linking tracker as
 * track_method (the reference's trackers are external MATLAB code).  Per class, up to max_tracks
 * times: anchor = best still-kept detection of the video (stop when its score < thres, :218);
 * link it frame by frame to the proposal with the highest float32 IoU with the current (int-
 * truncated) box while that IoU >= link_thres, at most ceil((max_frames+1)/2) frames per side
 * (max_frames <= 0: no limit; vdet/track.py:64-78); then, for every tracked box, track_det_nms
 * (utils/nms.pyx:128-189, threshold nms_thres) prunes that frame's still-kept detections.
 *   d_boxes [F,B,4] f32, d_scores [F,B,C] f32 (class innermost)
 *   d_tracks  [C,max_tracks,F,5] f32 rows (x1,y1,x2,y2,score), NaN where a track has no box
 *   d_anchors [C,max_tracks,3] f32 (1-based frame, box index, score);  d_ntracks [C] int32
 * Asynchronous after the graph build; failures are latched for vdet_sync.
 */
int vdet_track_volume(vdet_ctx *ctx, const float *d_boxes, const float *d_scores, int64_t F, int64_t B,
                      int64_t C, double nms_thres, double thres, int max_tracks, double link_thres,
                      int max_frames, float *d_tracks, float *d_anchors, int32_t *d_ntracks);

/*
 * vdet_track_volume that also returns the per-(frame, class) NMS survivors of vdet_nms_volume
 * (layout FBC, no score threshold, capacity `cap`: d_keep_idx [F,C,cap] int32 in descending score
 * order, d_keep_cnt [F,C]; VDET_ECAP latched like vdet_nms_volume) -- the detections
 * apply_image_nms (vdet/image_det.py:117-123) keeps for every frame next to the tubelets
 * greedily_track_from_raw_dets (vdet/track.py:189-252) builds from the same raw detections.
 * One call because both consume the same per-(frame, class) sorted lists and the same suppression
 * graph, which are built once.  Results are bit-identical to
 * calling vdet_nms_volume and vdet_track_volume separately.  d_keep_cnt == NULL: no NMS output.
 */
int vdet_nms_track_volume(vdet_ctx *ctx, const float *d_boxes, const float *d_scores, int64_t F, int64_t B,
                          int64_t C, double nms_thres, double thres, int max_tracks, double link_thres,
                          int max_frames, float *d_tracks, float *d_anchors, int32_t *d_ntracks, int64_t cap,
                          int32_t *d_keep_idx, int32_t *d_keep_cnt);

/*
 * Re-scoring of the device tracks: raw_dets_spatial_max_pooling (vdet/tubelet_cls.py:493-535: for
 * every tubelet box the best-scoring detection of its frame with float64 iou > overlap_thres gives
 * det_score and replaces the box -- the "box regression"), do_score_completion (:284-303) and
 * score_proto_temporal_maxpool(window) (:386-414; window 1 = none).
 *   d_tracks [C,T,F,5], d_ntracks [C] as produced by vdet_track_volume
 *   d_det_score [C,T,F] f64: completed spatial-max-pool score;  d_pooled [C,T,F] f64: after the
 *   temporal max-pool;  d_boxes_out [C,T,F,4] f32;  NaN where a track has no box.
 * Latches VDET_EINDEX where the reference raises IndexError (a tubelet without any overlapping
 * detection).
 */
int vdet_rescore_tracks(vdet_ctx *ctx, const float *d_tracks, const int32_t *d_ntracks, const float *d_boxes,
                        const float *d_scores, int64_t F, int64_t B, int64_t C, int max_tracks,
                        double overlap_thres, int window, double *d_det_score, double *d_pooled,
                        float *d_boxes_out);

/* ---- device evaluator (vdetlib_amd/eval.py on the GPU; ops.DetEvaluator) --------------------------------------------
 *
 * Per-class AP / mAP of detections against ground truth, with eval.py's evaluate() as the specification (bit for bit in
 * the matching, AP up to the order of one f64 sum).  A caller-owned STREAM of (class slot i32, score f64, tp u8) entries
 * collects the matched detections of every add; restricted to one class, its order is the order eval.py's adapters list
 * the detections in (tubelets (t, f), keep lists (f, k), video after video), so the stable sort of vdet_eval_ap
 * reproduces Python's stable sorted().  Class slots: the caller maps its evaluated classes to 0..K-1 (h_col_slot[c] for
 * score column c; -1 = class not evaluated, its detections are dropped).  rule 0 = VOC (IoU >= iou_thr, arg-max over the
 * unmatched ground truths, used ones count -1), 1 = ILSVRC VID (per-box threshold min(iou_thr, wh/((w+10)(h+10)))).
 *
 * Ground truth: a CSR built once (vdet_eval_gt_upload) from per-box (video index, frame, class slot, box f64) rows in
 * annotation order; h_vid_nf[v] = frames of video v in the table (boxes of frame >= nf, of a slot outside [0, K) or of a
 * video outside [0, NV) are not stored -- they can never match but still count in the caller's n_gt).
 *   d_gt_boxes [G,4] f64 (capacity G), d_gt_off [sum_v nf_v*K + 1] i32, d_vid_meta [NV,2] i64.  Synchronous.
 * Match calls enqueue one match launch and the order-preserving compaction, append at d_st_*[st_len ..] (capacity st_cap
 * must hold st_len + every candidate position of the call) and wait once: *h_count = entries appended.
 * vid: the detections' video in the table, -1 = unknown (every detection a false positive).
 */
int vdet_eval_gt_upload(vdet_ctx *ctx, const int32_t *h_vid, const int64_t *h_frame, const int32_t *h_slot, const double *h_boxes,
                        int64_t G, const int64_t *h_vid_nf, int64_t NV, int K, double *d_gt_boxes, int32_t *d_gt_off,
                        int64_t *d_vid_meta);

/* Tubelets of one video (vdet_track_volume / vdet_rescore_tracks outputs): d_boxes [C,T,F,box_stride] f32 (5: the track
 * rows, 4: d_boxes_out), d_scores [C,T,F] f64 (scores_f64) or f32, NaN = no box; tracks t >= d_ntracks[c] are skipped.
 * Frame f of the volume is frame f + 1 of the table. */
int vdet_eval_match_tracks(vdet_ctx *ctx, const double *d_gt_boxes, const int32_t *d_gt_off, const int64_t *d_vid_meta, int K,
                           int rule, double iou_thr, int vid, int64_t F, int64_t C, int T, const float *d_boxes, int box_stride,
                           const void *d_scores, int scores_f64, const int32_t *d_ntracks, const int32_t *h_col_slot,
                           int32_t *d_st_slot, double *d_st_score, uint8_t *d_st_tp, int64_t st_len, int64_t st_cap,
                           int64_t *h_count);

/* vdet_video_batch's tubelets of V videos in ONE match launch: video v's arrays start at element C*T*h_frame_off[v]
 * ([C,T,F_v] like vdet_eval_match_tracks), d_ntracks [V,C], h_vid [V] its table indices. */
int vdet_eval_match_tracks_batch(vdet_ctx *ctx, const double *d_gt_boxes, const int32_t *d_gt_off, const int64_t *d_vid_meta,
                                 int K, int rule, double iou_thr, const int32_t *h_vid, const int64_t *h_frame_off, int64_t V,
                                 int64_t C, int T, const float *d_boxes, int box_stride, const void *d_scores, int scores_f64,
                                 const int32_t *d_ntracks, const int32_t *h_col_slot, int32_t *d_st_slot, double *d_st_score,
                                 uint8_t *d_st_tp, int64_t st_len, int64_t st_cap, int64_t *h_count);

/* NMS survivors (vdet_nms_volume[_topk] / vdet_nms_track_volume / vdet_video_batch): d_boxes [F,B,4], d_scores [F,B,C] or
 * [F,C,B] f32, d_keep_idx [F,C,cap], d_keep_cnt [F,C].  Every list is walked in its own order; a list that is not
 * non-increasing in score, a kept NaN score or a count / index out of range latches VDET_EINVAL (vdet_sync). */
int vdet_eval_match_keep(vdet_ctx *ctx, const double *d_gt_boxes, const int32_t *d_gt_off, const int64_t *d_vid_meta, int K,
                         int rule, double iou_thr, int vid, const float *d_boxes, const float *d_scores, int layout, int64_t F,
                         int64_t B, int64_t C, const int32_t *d_keep_idx, const int32_t *d_keep_cnt, int64_t cap,
                         const int32_t *h_col_slot, int32_t *d_st_slot, double *d_st_score, uint8_t *d_st_tp, int64_t st_len,
                         int64_t st_cap, int64_t *h_count);

/* AP of every class slot over a stream of n entries: stable LSD radix sort by (slot asc, score desc; -0.0 == +0.0), then
 * per slot eval.py's average_precision with n_gt = d_ngt[k] (<= 0: NaN).  d_ap [K] f64.  d_perm [n] i32 or NULL: the
 * sorted order (stream positions).  Asynchronous. */
int vdet_eval_ap(vdet_ctx *ctx, const int32_t *d_st_slot, const double *d_st_score, const uint8_t *d_st_tp, int64_t n, int K,
                 const int64_t *d_ngt, double *d_ap, int32_t *d_perm);

/* ---- device TCN: the tubelet temporal-convolution scorer (score_conv_cls, vdet/tubelet_cls.py:15-51) ----------------------
 *
 * The net (vdetlib_amd/vdet/tcn.py: 1-D "same" convolutions over the tubelet length, ReLU between layers, a 2-way channel
 * softmax at the end) travels with every call: h_layers [n_layers][3] = (Cout, Cin, K) and h_params = W0 | b0 | W1 | b1 ...
 * (W [Cout,Cin,K] row-major, f32).  The context keeps the parameters of the last net on the device and uploads only when
 * the bytes differ (vdet_query(ctx, 10)).  Arithmetic = vdet_conv1d_f32's, element for element (acc = b[co]; ci outer, k
 * inner; acc = acc + w*x in f32 without contraction; zero padding at the ends of the series), so the results equal the
 * layer-by-layer path bit for bit, whichever of the paths of the limits table runs.
 *
 * Tubelet (c, t): the frames of d_tracks[c, t] whose row is not NaN (column 0), in frame order, compacted (length L);
 * t >= d_ntracks[c] does not exist.  h_channels [n_channels] selects and orders the net's input channels, one value per
 * box, rounded once from f64 to f32 like np.asarray(python floats, dtype='float32'):
 *   0 det_scores   d_det_score [C,T,F] (f64 when det_f64, else f32)        1 track_scores  d_tracks[..., 4]
 *   2 anchors      (frame - anchor frame) / L in f64, anchor frame = (int)d_anchors[c, t, 0] (1-based)
 *   3 abs_anchors  its magnitude        4 gt_overlaps  d_gt_overlap [C,T,F] f64        5 labels  gt_overlap >= 0.5 as 0 / 1
 * (4 / 5 without a d_gt_overlap buffer: VDET_EINVAL).  d_conv_score [C,T,F] f32 = probs[1] at the box's frame, NaN where
 * the tubelet has no box.  One assembly launch + one network launch; asynchronous, no host wait (a context that changes
 * nets or batch geometries between calls waits once per change for the copy of the previous table).
 */
int vdet_tcn_tracks(vdet_ctx *ctx, const float *h_params, const int32_t *h_layers, int n_layers, const int32_t *h_channels,
                    int n_channels, int64_t F, int64_t C, int T, const float *d_tracks, const int32_t *d_ntracks,
                    const float *d_anchors, const void *d_det_score, int det_f64, const double *d_gt_overlap, float *d_conv_score);

/* The same for the V videos of vdet_video_batch's layout in ONE assembly launch and ONE network launch: video v's arrays
 * start at element C*T*h_frame_off[v] and are [C,T,F_v]; d_ntracks [V,C], d_anchors [V,C,T,3]. */
int vdet_tcn_tracks_batch(vdet_ctx *ctx, const float *h_params, const int32_t *h_layers, int n_layers, const int32_t *h_channels,
                          int n_channels, const int64_t *h_frame_off, int64_t V, int64_t C, int T, const float *d_tracks,
                          const int32_t *d_ntracks, const float *d_anchors, const void *d_det_score, int det_f64,
                          const double *d_gt_overlap, float *d_conv_score);

/* The same scorer for nets whose inputs include WIDE blobs: per-box rows such as all_scores (the 200 SVM class scores of the
 * box) or feats (its pool5 feature, 1024 values), the second kind of input of score_conv_cls (vdet/tubelet_cls.py:35-41).
 * Input i of the n_inputs (1 .. 16, in the net's input order, one-channel and wide together) is
 *   h_codes[i] = 0 .. 5   an assembled channel as above; h_widths[i] must be 1, h_rows[i] / h_dtypes[i] are ignored;
 *   h_codes[i] = -1       a wide blob of h_widths[i] channels (1 .. 4096): h_rows[i] is a DEVICE pointer to contiguous rows
 *                         [C,T,F,W] in the box order of d_tracks (batch: video v's rows start at box C*T*h_frame_off[v],
 *                         i.e. one flat [C*T*Ftotal, W] array), h_dtypes[i] their storage: 0 f32 (taken as it is), 1 f16,
 *                         2 bf16 (both widened exactly), 3 f64 (rounded once to f32, like np.asarray(.., dtype='float32')).
 * Layer 0 sees Cin = the sum of the widths (<= 4096), concatenated in input order: channel q of a wide blob at series
 * position j is entry q of the row of the tubelet's j-th box.  A row is read only where the tubelet has a box
 * (t < d_ntracks[c] and column 0 of the track row is not NaN); rows of holes and of slots behind d_ntracks are never read,
 * whatever they hold; NaN / Inf inside a row that is read propagates as the arithmetic dictates.  Row bases need only element
 * alignment.  Arithmetic = vdet_conv1d_f32's, element for element, as above: bit-identical to the layer-by-layer path on
 * the same [Cin, L] input.  Layer 0 runs in a kernel of its own that reads the rows where they lie (no transposed or
 * compacted copy) and writes [Cout0, L] into a buffer of the context; the net kernel above runs the remaining layers (none
 * for a one-layer net: the softmax only).  VDET_EINVAL: n_inputs outside 1 .. 16, an unknown code or dtype, a null row
 * pointer, a width outside its range or unequal to layer 0's share (sum of widths != Cin of h_layers[0]), Cin > 4096.
 * One assembly launch + two network launches; asynchronous, no host wait (a call whose row pointers, widths or order
 * differ from the previous call's waits once for the copy of the previous input table, like a change of nets).
 */
int vdet_tcn_tracks_wide(vdet_ctx *ctx, const float *h_params, const int32_t *h_layers, int n_layers, const int32_t *h_codes,
                         const int32_t *h_widths, const void *const *h_rows, const int32_t *h_dtypes, int n_inputs, int64_t F,
                         int64_t C, int T, const float *d_tracks, const int32_t *d_ntracks, const float *d_anchors,
                         const void *d_det_score, int det_f64, const double *d_gt_overlap, float *d_conv_score);

int vdet_tcn_tracks_wide_batch(vdet_ctx *ctx, const float *h_params, const int32_t *h_layers, int n_layers,
                               const int32_t *h_codes, const int32_t *h_widths, const void *const *h_rows,
                               const int32_t *h_dtypes, int n_inputs, const int64_t *h_frame_off, int64_t V, int64_t C, int T,
                               const float *d_tracks, const int32_t *d_ntracks, const float *d_anchors, const void *d_det_score,
                               int det_f64, const double *d_gt_overlap, float *d_conv_score);

/* The network kernel on T ragged host series: series t is h_x[cin*h_off[t] ...], channel-major [cin, L_t] with
 * L_t = h_off[t+1] - h_off[t]; h_out[h_off[t] + j] = probs[1] of position j.  Synchronous: one upload, one launch, one
 * download for all series. */
int vdet_tcn_series_f32(vdet_ctx *ctx, const float *h_params, const int32_t *h_layers, int n_layers, int cin, const float *h_x,
                        const int64_t *h_off, int64_t T, float *h_out);

/* Ground-truth overlap of device tubelets (tubelets_overlap, utils/protocol.py:467-489) over the evaluator's table
 * (vdet_eval_gt_upload; frame f of the volume is frame f + 1 of the table, h_col_slot[c] the class slot of column c):
 *   d_gt_overlap [C,T,F] f64  the largest IoU (utils/common.py:451-468, vdet_iou_f64's operation order, ground truth first)
 *                             of the box with the ground-truth boxes of its video, frame and class; 0 when there is none
 *                             (or the video is unknown: vid -1); NaN where the tubelet has no box;
 *   d_mean_iou [C,T] f64      the mean over the tubelet's boxes, summed sequentially in frame order (NaN: no tubelet);
 *   d_gt [C,T] i32            |mean - 1| < DBL_EPSILON (a tubelet lying on a ground-truth track).
 * The box: d_tracks[..., :4], or d_boxes [C,T,F,4] when not NULL (vdet_rescore_tracks' d_boxes_out); d_tracks always says
 * where a tubelet has a box.  The f32 coordinates are widened to f64 AS THEY ARE -- the values vdet_eval_match_tracks
 * matches -- whereas ops.tracks_to_proto truncates them with int(): on integer-valued boxes the two agree bit for bit, on
 * fractional boxes the device form is the overlap of the untruncated box.  Asynchronous. */
int vdet_tubelets_overlap(vdet_ctx *ctx, const double *d_gt_boxes, const int32_t *d_gt_off, const int64_t *d_vid_meta, int K,
                          int vid, int64_t F, int64_t C, int T, const float *d_tracks, const float *d_boxes,
                          const int32_t *d_ntracks, const int32_t *h_col_slot, double *d_gt_overlap, double *d_mean_iou,
                          int32_t *d_gt);

/* V videos in vdet_video_batch's layout, one launch: h_vid [V] table indices, d_ntracks [V,C], d_mean_iou / d_gt [V,C,T]. */
int vdet_tubelets_overlap_batch(vdet_ctx *ctx, const double *d_gt_boxes, const int32_t *d_gt_off, const int64_t *d_vid_meta,
                                int K, const int32_t *h_vid, const int64_t *h_frame_off, int64_t V, int64_t C, int T,
                                const float *d_tracks, const float *d_boxes, const int32_t *d_ntracks, const int32_t *h_col_slot,
                                double *d_gt_overlap, double *d_mean_iou, int32_t *d_gt);

/* ---- device interpolation: strided / holey tubelets back to every frame (score_proto_interpolation,
 *      vdet/tubelet_cls.py:416-490) -----------------------------------------------------------------------------------------
 *
 * The inputs live on a SAMPLED frame axis of Fs rows (vdet_track_volume / vdet_rescore_tracks run on every stride-th frame
 * of the video, or any [C,T,Fs,...] tubelets with NaN rows); row i is the dense 1-based frame h_frames[i] (strictly
 * ascending, >= 1, <= F; NULL: i + 1, which needs F >= Fs).  The outputs live on the dense axis of F frames.
 * KNOTS of slot (c, t): the rows whose d_tracks column 0 is not NaN, t < d_ntracks[c].  With L knots:
 *   L == 0 (or t >= d_ntracks[c], whatever the rows hold)   every output NaN;
 *   L == 1   the one box copied to its frame, NaN elsewhere (the reference copies tubelets of < 2 boxes, :452-454);
 *   L >= 2   frames lo..hi, lo / hi = first / last knot frame with the end rule lo == 2 -> 1, hi == F - 1 -> F
 *            (:472-475), NaN elsewhere.  Arithmetic = vdet_series_interp_f64's in f64, operation for operation, without
 *            contraction: the knot's own value at a knot; else slope = (y[j+1]-y[j])/(x[j+1]-x[j]), slope*(x-x[j]) + y[j]
 *            from the LEFT knot; frame 1 below the knots y[0] + (x-x[0])*(y[1]-y[0])/(x[1]-x[0]); frame F above them
 *            y[-1] + (x-x[-1])*(y[-1]-y[-2])/(x[-1]-x[-2]).  A NaN in a knot's field flows through that arithmetic.
 * Fields, all interpolated by that one rule:
 *   the box        d_boxes [C,T,Fs,4] f32 when not NULL (vdet_rescore_tracks' d_boxes_out), else d_tracks[..., :4]; the
 *                  f32 values widened to f64 AS THEY ARE (no int(), as in vdet_tubelets_overlap)
 *                  -> d_boxes64 [C,T,F,4] f64;  d_tboxes [C,T,F,4] f32 and d_tracks_out[..., :4] = that, rounded once
 *   n_series <= 4  h_series[q]: DEVICE pointers [C,T,Fs], all f64 (series_f64) or all f32 -- each a det_score field of the
 *                  reference -> d_series_out [n_series][C*T*F] f64 (batch: F = all dense frames of the call): series q
 *                  starts at element q*C*T*F and is laid out like every other [C,T,F] output
 *   the anchor     h_frames[i] - h_frames[(int)d_anchors[c,t,0] - 1], the offset in dense frames (the reference's
 *                  tracks_proto_from_boxes(..., start_frame, step)) -> d_anchor [C,T,F] f64 (NaN when the anchor row is
 *                  not a row of the video)
 *   track score    d_tracks[..., 4] -> d_tracks_out[..., 4] f32, rounded once.  BUILD-DEFINED: the reference's interpolated
 *                  boxes carry no track_score; the device TCN reads one per box, so it is interpolated like a score.
 * d_tracks_out [C,T,F,5] rows are NaN exactly where the tubelet has no dense box.  d_anchors_out [C,T,3] f32: column 0 is
 * the anchor's dense frame number (copied unchanged for t >= d_ntracks[c] or an anchor row outside the video), columns 1-2
 * copied.  Every output element is written by the ONE launch of the call (no fill pass).  Asynchronous, no host wait
 * (h_frames and the offsets are staged in the context; a change of table waits once for the copy of the previous one).
 */
int vdet_interp_tracks(vdet_ctx *ctx, int64_t Fs, int64_t F, const int32_t *h_frames, int64_t C, int T, const float *d_tracks,
                       const float *d_boxes, const int32_t *d_ntracks, const float *d_anchors, const void *const *h_series,
                       int n_series, int series_f64, float *d_tracks_out, double *d_boxes64, float *d_tboxes,
                       double *d_series_out, double *d_anchor, float *d_anchors_out);

/* The same for V videos in vdet_video_batch's layout, one launch: the inputs of video v start at element
 * C*T*h_sframe_off[v] and are [C,T,Fs_v], its outputs at C*T*h_frame_off[v] and are [C,T,F_v]; h_frames [h_sframe_off[V]]
 * (ascending inside each video, or NULL), d_ntracks [V,C], d_anchors / d_anchors_out [V,C,T,3]. */
int vdet_interp_tracks_batch(vdet_ctx *ctx, const int64_t *h_sframe_off, const int64_t *h_frame_off, int64_t V,
                             const int32_t *h_frames, int64_t C, int T, const float *d_tracks, const float *d_boxes,
                             const int32_t *d_ntracks, const float *d_anchors, const void *const *h_series, int n_series,
                             int series_f64, float *d_tracks_out, double *d_boxes64, float *d_tboxes,
                             double *d_series_out, double *d_anchor, float *d_anchors_out);

/* ---- device anchor route: tubelets from caller-supplied anchors (track_from_det, vdet/track.py:109-119) and the anchor
 *      detection's score on every box of the tubelet (anchor_propagate, vdet/tubelet_cls.py:353-383) ---------------------
 *
 * vdet_track_from_anchors: slot (c, t) of d_anchor_frames [C,T] int32 (1-based frame, 0 = empty slot) / d_anchor_boxes
 * [C,T,4] f32 / d_anchor_scores [C,T] f32 (or NULL) is one anchor; C is only a grouping axis (linking does not depend on
 * the class).  The tubelet of a live slot is what vdet_track_volume's built-in tracker makes from that BOX: the anchor row
 * is (int-truncated box, 1.0); the chain runs forward, then backward; a step scores every box of the next frame with the
 * f32 IoU of utils/nms.pyx (the current box as the "i" box), NaN IoUs are out of the running, the best wins, ties go to
 * the lowest box index; it stops when every IoU is NaN, when the best is < link_thres, at the video's end or after
 * ceil((max_frames+1)/2) - 1 steps (max_frames <= 0: no limit); the new current box is the truncated proposal, its row
 * (truncated box, IoU).  Rows not reached are NaN.
 *   d_tracks  [C,T,F,5] f32   every row written by the ONE launch of the call (no fill pass); all NaN for an empty slot
 *   d_anchors [C,T,3]   f32   (frame, -1, score or 0)
 *   d_ntracks [C]       int32 1 + the last live slot of the class (an empty slot below it is a tubelet without boxes)
 * An anchor frame outside 0..F is latched (VDET_EINVAL at vdet_sync); its slot is written as an empty one.  Asynchronous, no
 * host wait, no host table.  Reads and writes nothing of the context's cached graph, lists, index or link memo.
 */
int vdet_track_from_anchors(vdet_ctx *ctx, const float *d_boxes, int64_t F, int64_t B, const int32_t *d_anchor_frames,
                            const float *d_anchor_boxes, const float *d_anchor_scores, int64_t C, int T, double link_thres,
                            int max_frames, float *d_tracks, float *d_anchors, int32_t *d_ntracks);

/* d_tracks / d_ntracks / d_anchors of vdet_track_from_anchors, vdet_track_volume or vdet_nms_track_volume; d_boxes [F,B,4],
 * d_scores [F,B,C] f32.  Slot (c, t), t < d_ntracks[c], fa = (int)d_anchors[c,t,0] in 1..F, anchor row not NaN:
 *   ov = utils/common.py:451-468 iou (f64, +1 convention, inter / (a1 + a2 - inter); a zero union is NaN as in numpy, not an
 *        error) of d_tracks[c,t,fa-1,:4] -- widened to f64 as it is -- against the B boxes of frame fa;
 *   d_best[c,t] = np.argmax(ov): the first maximum, a NaN counts as the maximum, the first NaN wins;
 *   d_det_score[c,t,f] = (double)d_scores[fa-1, best, c] on every frame whose track row is not NaN, NaN elsewhere.
 * Every other slot (t >= d_ntracks[c], frame 0, a NaN anchor row): d_det_score NaN, d_best -1.  A live slot whose anchor
 * frame is neither 0 nor in 1..F is latched (VDET_EINVAL at vdet_sync).  One launch writes every output element. */
int vdet_anchor_propagate_tracks(vdet_ctx *ctx, const float *d_tracks, const int32_t *d_ntracks, const float *d_anchors,
                                 const float *d_boxes, const float *d_scores, int64_t F, int64_t B, int64_t C, int T,
                                 double *d_det_score, int32_t *d_best);

/* The arg-max of the dict-level anchor_propagate on host tables, all anchors of a call in one launch (synchronous):
 * h_best[n] = np.argmax(iou([h_anchor_boxes[n]], h_det_boxes[h_group_off[g] .. h_group_off[g+1]))), g = h_group[n] the
 * anchor's frame slot; -1 for a frame slot without detections.  All f64. */
int vdet_anchor_argmax_f64(vdet_ctx *ctx, const double *h_anchor_boxes, const int32_t *h_group, int64_t N,
                           const double *h_det_boxes, const int64_t *h_group_off, int64_t G, int64_t *h_best);

/* ---- device anchor selection: top_detections / frame_top_detections (utils/protocol.py:330-351) as arrays, every class
 *      (and every video of a batch) in one call; its outputs are vdet_track_from_anchors' inputs -------------------------
 *
 * d_boxes [F,B,4] f32 (16-byte aligned), d_scores [F,B,C] f32, class innermost.  A candidate of class c is a detection whose
 * score is not NaN and -- use_score_thresh != 0 -- is > (float)score_thresh (f32 compare, as vdet_nms_volume_topk).  Candidates
 * are ordered by descending score, equal scores (-0.0 == +0.0) by ascending flat index f*B + b (Python's stable
 * sorted(..., reverse=True) over a frame-major proto).  NOT mirrored: the reference returns a proto of fewer than top_num
 * detections unsorted; this call always sorts.
 *   mode 0 (video): T = top_num <= 1024; slot (c, t) is the t-th candidate of class c.  h_frame_off = NULL: one video, outputs
 *     [C,T]; no host table.  h_frame_off [V+1]: V videos, outputs [V,C,T], the selection runs inside each video's frames and
 *     frames are local to the video (as vdet_video_batch's anchors).
 *   mode 1 (frame): top_num <= 128, T = F*top_num, outputs [C,T]; slot (c, f*top_num + r) is the r-th candidate of frame f.
 *     h_frame_off must be NULL.
 *   d_anchor_frames int32 (1-based, 0 = empty slot), d_anchor_boxes [..,4] f32 (the proposal's box as it is: the link call
 *   truncates), d_anchor_scores f32, d_anchor_index int32 (box index in its frame, -1 = empty).  An empty slot's box and score
 *   are 0.  Every element is written by the call's own kernels (no fill pass).
 * Asynchronous: no host wait; the single-video and frame forms stage no host table, the batch form the per-video table keyed
 * by the offsets (vdet_query 11).  Scratch is O(V*C*(256 + segments + T)): no transposed or keyed copy of the volume.  Reads
 * and writes nothing of the context's cached graph, lists, index or link memo. */
int vdet_top_anchors(vdet_ctx *ctx, const float *d_boxes, const float *d_scores, int64_t F, int64_t B, int64_t C, int top_num,
                     int mode, int use_score_thresh, double score_thresh, const int64_t *h_frame_off, int64_t V,
                     int32_t *d_anchor_frames, float *d_anchor_boxes, float *d_anchor_scores, int32_t *d_anchor_index);

/* vdet_track_from_anchors for V videos in ONE launch: d_boxes [Ftot,B,4] holds the videos' frames one after the other
 * (h_frame_off [V+1]); d_anchor_frames [V,C,T] (1-based inside the video) / d_anchor_boxes [V,C,T,4] / d_anchor_scores [V,C,T] or
 * NULL.  A chain stops at its own video's first and last frame.  Outputs in vdet_video_batch's layout: d_tracks is one flat
 * buffer of C*T*Ftot*5 floats, video v's [C,T,F_v,5] block at element C*T*5*h_frame_off[v]; d_anchors [V,C,T,3]; d_ntracks
 * [V,C].  Per video the bits are vdet_track_from_anchors' on that video alone.  An anchor frame outside 0..F_v is latched
 * (VDET_EINVAL at vdet_sync), its slot written as an empty one.  The per-video table is staged keyed by the offsets: the same
 * offsets again neither wait nor copy. */
int vdet_track_from_anchors_batch(vdet_ctx *ctx, const float *d_boxes, const int64_t *h_frame_off, int64_t V, int64_t B,
                                  const int32_t *d_anchor_frames, const float *d_anchor_boxes, const float *d_anchor_scores,
                                  int64_t C, int T, double link_thres, int max_frames, float *d_tracks, float *d_anchors,
                                  int32_t *d_ntracks);

/* vdet_anchor_propagate_tracks for V videos in ONE launch, on the buffers of vdet_track_from_anchors_batch / vdet_video_batch:
 * d_det_score is flat, video v's [C,T,F_v] block at element C*T*h_frame_off[v]; d_best [V,C,T]. */
int vdet_anchor_propagate_tracks_batch(vdet_ctx *ctx, const float *d_tracks, const int32_t *d_ntracks, const float *d_anchors,
                                       const float *d_boxes, const float *d_scores, const int64_t *h_frame_off, int64_t V,
                                       int64_t B, int64_t C, int T, double *d_det_score, int32_t *d_best);

/* ---- device merge: two scored tubelet sets into one (merge_score_protos, utils/protocol.py:504-525) ------------------------
 *
 * A tubelet SET of one video: d_tracks [C,T,F,5] f32, d_ntracks [C] i32, d_anchors [C,T,3] f32, optionally d_tboxes [C,T,F,4]
 * f32, and n_series (1..4) series [C,T,F] f64 whose DEVICE pointers sit in the host arrays h_series_a / h_series_b; series 0
 * is det_score.  A box exists where d_tracks[c,t,f,0] is not NaN and t < d_ntracks[c] -- the rule of every other stage; counts
 * outside 0..T are clamped.  Sets a and b share C, F, n_series and the presence of tboxes (d_tboxes_a, d_tboxes_b and
 * d_tboxes_out: all given or all NULL); Ta and Tb may differ.  Inputs are never modified; a and b may be the same buffers.
 *
 * VDET_MERGE_COMBINE (:510-511, list extend: a's tubelets, then b's).  T_out = Ta + Tb.  For class c, out slot t < nta[c] is a's
 *   slot t, out slot nta[c] + u (u < ntb[c]) is b's slot u, d_ntracks_out[c] = nta[c] + ntb[c].  Live slots are copied bit for
 *   bit in every field (rows, tboxes, all series, anchors), empty slots below ntracks included.  Every slot at or behind
 *   d_ntracks_out[c] is written as NaN rows, NaN tboxes, NaN series and a zero anchor, whatever the inputs hold there.
 *   d_from_b is not written (NULL).
 * VDET_MERGE_MAX (:512-524).  The output has a's shape: T_out = Ta, d_ntracks_out = nta.  Slots t >= min(nta[c], ntb[c]) are
 *   copies of a (zip over the tubelet lists).  Inside a paired slot the reference zips the two box lists: with ca / cb boxes and
 *   m = min(ca, cb), the i-th box of a meets the i-th box of b for i < m.  The two must lie on the same frame (assert
 *   box1['frame'] == box2['frame']) and, when m >= 1, the integer anchor frames (int)d_anchors[c,t,0] of the two slots must be
 *   equal (assert box1['anchor'] == box2['anchor']).  Where det_b > det_a (the f64 compare of box1['det_score'] <
 *   box2['det_score']: a NaN on either side, equal scores and -0.0 against +0.0 keep a) b's values are taken for every field a's
 *   box has: the row (box and track score), tboxes and all series.  Boxes of a with ordinal >= m are unchanged; anchors are a's.
 *   d_from_b [C,Ta,F] u8: 1 where b's box was taken, 0 elsewhere.  A slot that violates an assertion latches VDET_EINVAL in the
 *   context's status word (reported by vdet_sync, as vdet_track_from_anchors' bad anchor frame) and is written as a copy of a;
 *   all other slots are unaffected.  The reference's `gt` and `class` assertions have no device counterpart: the sets carry no
 *   gt flag, and the class of a slot is its index c on both sides.
 * d_series_out [n_series][C*T_out*F] f64: series q starts at element q*C*T_out*F (batch: F = all frames of the call) and is laid
 * out like every other [C,T,F] output.  Every output element is written by the ONE launch of the call (no fill pass).
 * Asynchronous: no host wait, no host table, no scratch; reads and writes nothing of the context's cached graph, lists, index
 * or link memo.
 */
#define VDET_MERGE_COMBINE 0
#define VDET_MERGE_MAX 1

int vdet_merge_tracks(vdet_ctx *ctx, int scheme, int64_t F, int64_t C, int Ta, int Tb,
                      const float *d_tracks_a, const int32_t *d_ntracks_a, const float *d_anchors_a, const float *d_tboxes_a,
                      const float *d_tracks_b, const int32_t *d_ntracks_b, const float *d_anchors_b, const float *d_tboxes_b,
                      const double *const *h_series_a, const double *const *h_series_b, int n_series, float *d_tracks_out,
                      int32_t *d_ntracks_out, float *d_anchors_out, float *d_tboxes_out, double *d_series_out, uint8_t *d_from_b);

/* The same for V videos in vdet_video_batch's layout, ONE launch with the video as a grid dimension: set a's arrays of video v
 * start at element C*Ta*h_frame_off[v] and are [C,Ta,F_v], set b's at C*Tb*h_frame_off[v], the outputs at C*T_out*h_frame_off[v];
 * d_ntracks_* [V,C], d_anchors_* [V,C,T,3].  Per video the bits are vdet_merge_tracks' on that video alone.  More than one video
 * reads the per-video table of the anchor route's batch forms, staged keyed by the offsets (vdet_query 11): the same offsets
 * again neither wait nor copy. */
int vdet_merge_tracks_batch(vdet_ctx *ctx, int scheme, const int64_t *h_frame_off, int64_t V, int64_t C, int Ta, int Tb,
                            const float *d_tracks_a, const int32_t *d_ntracks_a, const float *d_anchors_a, const float *d_tboxes_a,
                            const float *d_tracks_b, const int32_t *d_ntracks_b, const float *d_anchors_b, const float *d_tboxes_b,
                            const double *const *h_series_a, const double *const *h_series_b, int n_series, float *d_tracks_out,
                            int32_t *d_ntracks_out, float *d_anchors_out, float *d_tboxes_out, double *d_series_out,
                            uint8_t *d_from_b);

/* ---- device NMS of tubelets with still-image detections, per frame and class (vid_nms, utils/nms.pyx:71-125) ---------------
 *
 * What apply_vid_nms (vdet/video_det.py:51-61) does to a detection proto: vid_nms never suppresses across frames, so it is one
 * nms (utils/nms.pyx:17-68) per (class, frame) list.  For every class c and frame f the candidate ROWS are, in this order:
 *   1. still-image rows (optional source: the four tensors vdet_eval_match_keep takes, layout [F,B,C] only).  For
 *      k in 0 .. min(d_keep_cnt[f,c], top_still) - 1, with b = d_keep_idx[f,c,k], the row is (d_boxes[f,b,0:4], d_scores[f,b,c]).
 *      Keep lists are in descending score order, so the prefix is the max_per_image cut of fast_rcnn_det_vid.  Entries behind
 *      the count are never read.  Without the source (top_still = 0) the four pointers are not read and may be NULL.
 *   2. tubelet rows.  For t in 0 .. d_ntracks[c] - 1 (clamped to 0..T) where d_tracks[c,t,f,0] is not NaN, the row is
 *      (box, (float)score[c,t,f]): box is d_tboxes[c,t,f] when d_tboxes is given, else d_tracks[c,t,f,0:4]; d_score is a [C,T,F]
 *      series of the caller's choice, f32 or f64 (score_f64), rounded to f32 to nearest.  Slots t >= d_ntracks[c] are never
 *      read, whatever they hold.  T = 0: no tubelet source, the pointers may be NULL.
 * A row whose f32 score is NaN is absent, from either source (the evaluator's "NaN = no box" rule).
 * The result of the list is nms(rows, thresh) with the conventions at the top of this file: f32 arithmetic, +1 areas,
 * suppression iff (double)ovr_f32 >= thresh; descending score, -0.0 == +0.0, equal scores by DESCENDING row index -- at equal
 * score a tubelet row therefore precedes a still-image row, and a higher slot a lower one.  A zero union of an EVALUATED pair
 * (a kept row against a still-alive one) latches VDET_EDIVZERO (vdet_sync); a pair the reference never evaluates raises
 * nothing.  NaN / inf coordinates behave as in every other NMS entry point (comparisons with NaN are false).
 *
 * Outputs, in the tubelet layout with the RANK as the slot axis (R rows; top_still + T can never overflow), so every consumer
 * of tubelets reads them unchanged (vdet_eval_match_tracks with box_stride 5 and the f64 score):
 *   d_tracks_out [C,R,F,5] f32   row r of frame f is the r-th kept detection (x1,y1,x2,y2, f32 score); NaN behind the count
 *   d_score_out  [C,R,F]   f64   the source's own score unrounded (f64 series as given, f32 widened); NaN behind the count
 *   d_src_out    [C,R,F]   i32   b >= 0: still-image box b of that frame; -(t+1): tubelet slot t; INT32_MIN behind the count
 *   d_cnt_out    [C,F]     i32   detections kept
 *   d_ntracks_out [C]      i32   max over f of min(cnt[c,f], R) (an integer atomic max)
 * More survivors than R latch VDET_ECAP: the count is still written, nothing is written past R.  A d_keep_cnt outside 0..cap
 * (the list then has no still-image rows) or a read d_keep_idx outside 0..B-1 (that row is skipped) latches VDET_EINVAL.
 * Inputs are never modified.  Every output element is written by the ONE launch of the call; asynchronous, no host wait, no
 * scratch; reads and writes nothing of the context's cached graph, lists, index or link memo.  d_boxes and d_tboxes must be
 * 16-byte aligned.  Limits: the table at the top of this file.
 */
int vdet_nms_tracks(vdet_ctx *ctx, int64_t F, int64_t C, int T, const float *d_tracks, const int32_t *d_ntracks, const void *d_score,
                    int score_f64, const float *d_tboxes, const float *d_boxes, const float *d_scores, int64_t B,
                    const int32_t *d_keep_idx, const int32_t *d_keep_cnt, int64_t cap, int top_still, double thresh, int R,
                    float *d_tracks_out, double *d_score_out, int32_t *d_src_out, int32_t *d_cnt_out, int32_t *d_ntracks_out);

/* The same for V videos in vdet_video_batch's layout, ONE launch with the video as a grid dimension.  The still-image tensors
 * are frame-major over all videos ([Ftot,...]); the tubelet arrays of video v start at element C*T*h_frame_off[v] and are
 * [C,T,F_v], the outputs at C*R*h_frame_off[v] ([C,R,F_v]); d_ntracks [V,C], d_cnt_out [C,Ftot], d_ntracks_out [V,C].  Per video
 * the bits are vdet_nms_tracks' on that video alone.  More than one video reads the per-video table of the anchor route's batch
 * forms, staged keyed by the offsets (vdet_query 11): the same offsets again neither wait nor copy. */
int vdet_nms_tracks_batch(vdet_ctx *ctx, const int64_t *h_frame_off, int64_t V, int64_t C, int T, const float *d_tracks,
                          const int32_t *d_ntracks, const void *d_score, int score_f64, const float *d_tboxes, const float *d_boxes,
                          const float *d_scores, int64_t B, const int32_t *d_keep_idx, const int32_t *d_keep_cnt, int64_t cap,
                          int top_still, double thresh, int R, float *d_tracks_out, double *d_score_out, int32_t *d_src_out,
                          int32_t *d_cnt_out, int32_t *d_ntracks_out);

/* ---- device Soft-NMS of the same lists: scores decayed, nothing deleted (Bodla et al., ICCV 2017) ---------------------------
 *
 * The reference has no such step; the rule is this file's, stated again in numpy float32 by tests/softnms_spec.py, which the
 * device equals on bits.  ROWS: vdet_nms_tracks' rows, in its order and with its row indices (still-image rows
 * k < min(d_keep_cnt, top_still), then tubelet rows by slot; a NaN f32 score is no row; a d_keep_cnt / d_keep_idx out of range
 * latches VDET_EINVAL and the entry is skipped).  Every row carries a CURRENT f32 score, at first the f32 rounding of its
 * source score.  With min32 = (float)min_score and sigma32 = (float)sigma:
 *   1. every row whose current score is < min32 is removed (min_score = -inf removes nothing);
 *   2. while a row is alive:
 *      - the alive row with the largest current score is taken: -0.0 == +0.0, equal scores by DESCENDING row index -- the order
 *        at the top of this file applied to the current scores;
 *      - it is EMITTED as the next rank: its box, its current score bit for bit (a -0.0 stays -0.0), its src; it is no longer
 *        alive;
 *      - for every other alive row j: ovr as utils/nms.pyx:57-64 computes it in f32 with the emitted box as box i ('/' is the
 *        correctly rounded division).  Every alive row is an EVALUATED pair: a zero union latches VDET_EDIVZERO (vdet_sync), as
 *        in vdet_nms_tracks.  A NaN ovr changes nothing.  Otherwise
 *          method 0 'linear':  iff (double)ovr >= thresh:  s_j = s_j * (1.0f - ovr)       two f32 operations
 *          method 1 'gauss':   s_j = s_j * g(-(ovr * ovr) / sigma32)   for every pair; thresh is not used
 *      - a score that became NaN (inf * 0) or fell below min32 removes the row.
 * '>=' is this project's convention for every threshold; Bodla's code tests ovr > thresh, so the two differ exactly where
 * ovr == thresh.
 * g is an exponential written as a fixed sequence of single, correctly rounded f32 operations (csrc/softnms_kernels.hpp sn_exp,
 * tests/softnms_spec.py g; the library is built with -ffp-contract=off): x < -87 gives +0.0; else x is rounded to a multiple
 * of 2^-20, k = rint(x * log2 e), r = x - k * ln2_hi - k * ln2_lo, a degree-6 polynomial in r by Horner's scheme, ldexp(p, k).
 * g(0) = 1 exactly, 0 <= g <= 1, g never increases as its argument falls (that is what the 2^-20 grid is for), and its
 * largest relative distance from exp over [-64, 0] is 6e-7.
 * The multiplicative rule is the published one and is meant for scores >= 0: a NEGATIVE score moves towards zero -- it RISES --
 * when it is decayed, and an infinite one stays infinite or, times 0, becomes NaN and is removed.  Nothing here "repairs" that:
 * mapping SVM margins into [0, 1] first is the caller's elementwise operation.
 *
 * Outputs: vdet_nms_tracks' rank layout.  d_tracks_out [C,R,F,5] holds the box and the DECAYED f32 score, d_score_out [C,R,F]
 * that score widened to f64, d_score0_out [C,R,F] f64 the source's own unrounded score (what vdet_nms_tracks writes to
 * d_score_out), d_src_out / d_cnt_out / d_ntracks_out as there, cnt = rows emitted.  More emitted rows than R latch VDET_ECAP:
 * the count is still written, nothing past R.  NaN / INT32_MIN behind the counts.  One round per emitted row, each
 * ceil(n / 64) f32 divisions per lane.
 * VDET_EINVAL before any launch, with nothing written: method other than 0 / 1; sigma not finite or below 1/64 (with
 * ovr <= 1 the argument of g then stays in [-64, 0], the range its accuracy is stated for); a NaN thresh or min_score; a NULL
 * d_score0_out; everything vdet_nms_tracks rejects.  Inputs are never modified.  Every output element is written by the ONE
 * launch of the call; asynchronous, no host wait, no scratch; reads and writes nothing of the context's cached graph, lists,
 * index or link memo.  Timed under "other".
 */
int vdet_soft_nms_tracks(vdet_ctx *ctx, int64_t F, int64_t C, int T, const float *d_tracks, const int32_t *d_ntracks,
                         const void *d_score, int score_f64, const float *d_tboxes, const float *d_boxes, const float *d_scores,
                         int64_t B, const int32_t *d_keep_idx, const int32_t *d_keep_cnt, int64_t cap, int top_still, double thresh,
                         int R, int method, double sigma, double min_score, float *d_tracks_out, double *d_score_out,
                         int32_t *d_src_out, int32_t *d_cnt_out, int32_t *d_ntracks_out, double *d_score0_out);

/* The same for V videos, laid out and staged as in vdet_nms_tracks_batch (d_score0_out like d_score_out); per video the bits
 * are vdet_soft_nms_tracks' on that video alone. */
int vdet_soft_nms_tracks_batch(vdet_ctx *ctx, const int64_t *h_frame_off, int64_t V, int64_t C, int T, const float *d_tracks,
                               const int32_t *d_ntracks, const void *d_score, int score_f64, const float *d_tboxes,
                               const float *d_boxes, const float *d_scores, int64_t B, const int32_t *d_keep_idx,
                               const int32_t *d_keep_cnt, int64_t cap, int top_still, double thresh, int R, int method, double sigma,
                               double min_score, float *d_tracks_out, double *d_score_out, int32_t *d_src_out, int32_t *d_cnt_out,
                               int32_t *d_ntracks_out, double *d_score0_out);

/* ---- device box voting on the same lists: NMS survivors take their neighbours' boxes (Gidaris & Komodakis, ICCV 2015) --------
 *
 * The reference has no such step; the rule is this file's, stated again in numpy by tests/votenms_spec.py, which the device
 * equals on bits.
 *   1. KEPT ROWS.  The list's rows, row indices, order, kept rows, ranks, score, src, cnt, ntracks and status flags are exactly
 *      vdet_nms_tracks' at thresh -- the VDET_EDIVZERO of a zero-union pair the hard NMS evaluates and the VDET_EINVAL of bad
 *      keep data included.
 *   2. VOTERS of the kept row i: i itself (no test), and every other PRESENT row j of the list -- not absent; suppressed rows
 *      and other kept rows are included -- that passes the overlap test: with ovr and uni computed exactly as
 *      utils/nms.pyx:57-64 computes them in f32 with i as box i, j votes iff uni != 0 and (double)ovr >= vote_thresh (the
 *      threshold goes through the same rounding-up to f32 as thresh).  A NaN ovr or a zero union is no voter and latches
 *      NOTHING: these are pairs the reference never evaluates.
 *   3. WEIGHTS.  weights 0 'score': w_j = (double)s32_j if s32_j > 0, else 0.0, s32 = the f32 score the NMS orders by.
 *      weights 1 'uniform': w_j = 1.0.
 *   4. SUMS.  sw and the four sx_k in float64, sequentially over the voters in ASCENDING row index, from 0.0; each step is
 *      sw += w_j; sx_k += w_j * (double)box_j[k] -- one correctly rounded multiply and one correctly rounded add (the library
 *      is built with -ffp-contract=off).
 *   5. RESULT.  If sw > 0 and all four sx_k / sw (correctly rounded f64 divisions) are finite, the row's box is
 *      (float)(sx_k / sw); otherwise the row keeps its own box.
 * A score <= 0 (or -0.0) makes a voter weigh nothing under 'score' -- its vote is still counted -- and a list of such rows keeps
 * its own boxes; an infinite score makes the quotient inf / inf and the row keeps its own box.  Nothing here "repairs" that:
 * mapping SVM margins into [0, 1] first is the caller's elementwise operation, as for vdet_soft_nms_tracks.
 * With vote_thresh > 1 no row but i votes, w * x is exact in float64, (w * x) / w == x, and every output vdet_nms_tracks also
 * has equals it bit for bit.  With thresh > 1 every row is kept and votes is a symmetric neighbourhood count.
 *
 * Outputs: vdet_nms_tracks' rank layout.  d_tracks_out [C,R,F,5] holds the VOTED box and the row's own f32 score, d_score_out
 * / d_src_out / d_cnt_out / d_ntracks_out as there; d_box0_out [C,R,F,4] f32 the row's own box (NaN behind the count),
 * d_votes_out [C,R,F] int32 the number of voters, the row itself included (0 behind the count).  More kept rows than R latch
 * VDET_ECAP: the count is still written, nothing past R.
 * VDET_EINVAL before any launch, with nothing written: weights other than 0 / 1; a NaN vote_thresh; a NULL d_box0_out or
 * d_votes_out; everything vdet_nms_tracks rejects.  Inputs are never modified.  Every output element is written by the ONE
 * launch of the call; asynchronous, no host wait, no scratch; reads and writes nothing of the context's cached graph, lists,
 * index or link memo.  One lane per kept row walks the list: ceil(min(cnt, R) / 64) * n pair tests per lane on top of the
 * selection's.  Timed under "other".
 */
int vdet_vote_nms_tracks(vdet_ctx *ctx, int64_t F, int64_t C, int T, const float *d_tracks, const int32_t *d_ntracks,
                         const void *d_score, int score_f64, const float *d_tboxes, const float *d_boxes, const float *d_scores,
                         int64_t B, const int32_t *d_keep_idx, const int32_t *d_keep_cnt, int64_t cap, int top_still, double thresh,
                         int R, double vote_thresh, int weights, float *d_tracks_out, double *d_score_out, int32_t *d_src_out,
                         int32_t *d_cnt_out, int32_t *d_ntracks_out, float *d_box0_out, int32_t *d_votes_out);

/* The same for V videos, laid out and staged as in vdet_nms_tracks_batch (d_box0_out like d_tracks_out with 4 floats a row,
 * d_votes_out like d_src_out); per video the bits are vdet_vote_nms_tracks' on that video alone. */
int vdet_vote_nms_tracks_batch(vdet_ctx *ctx, const int64_t *h_frame_off, int64_t V, int64_t C, int T, const float *d_tracks,
                               const int32_t *d_ntracks, const void *d_score, int score_f64, const float *d_tboxes,
                               const float *d_boxes, const float *d_scores, int64_t B, const int32_t *d_keep_idx,
                               const int32_t *d_keep_cnt, int64_t cap, int top_still, double thresh, int R, double vote_thresh,
                               int weights, float *d_tracks_out, double *d_score_out, int32_t *d_src_out, int32_t *d_cnt_out,
                               int32_t *d_ntracks_out, float *d_box0_out, int32_t *d_votes_out);

/* ---- device re-scoring of ANY tubelet set against the detections -----------------------------------------------------------
 *
 * raw_dets_spatial_max_pooling (vdet/tubelet_cls.py:493-535), then do_score_completion (:284-303), then
 * score_proto_temporal_maxpool (:386-414) for tubelets of any origin -- caller-supplied, anchor-route, merged, interpolated --
 * and, with a FLOOR, the part of rcnn_sampling_dets_scoring (:221-259) that follows the CNN.  vdet_rescore_tracks and
 * vdet_video_batch keep their own kernels, which assume the greedy tracker's contiguous tubelets; this entry point treats a
 * tubelet as the reference does, as the LIST of its boxes.
 *
 * Layout (vdet_video_batch's): video v's [C,T,F_v,5] tracks start at element C*T*5*h_frame_off[v] of one flat buffer;
 * d_ntracks [V,C], d_boxes [F,B,4], d_scores [F,B,C] over all frames.  d_floor, d_det, d_pooled, d_src are [C,T,F_v] per video at
 * C*T*h_frame_off[v], d_tboxes [C,T,F_v,4].  d_floor may be NULL; it is f64 when floor_f64, else f32.
 *
 * A tubelet box is PRESENT when t < d_ntracks[v,c] and the row's x1 is not NaN.  Everything else gets NaN in det, pooled and
 * tboxes and -1 in src.
 *
 * Spatial step, per present box.  Candidates: the detections j of the same frame with f64 iou(row, box_j) > overlap_thres
 * (strict; the f32 values widened to f64; utils/common.py:451-468).  best = numpy's argmax of their class scores: the first
 * maximum, a NaN counts as the maximum.
 *   no floor:  a hit gives det = score, tbox = the detection's box, src = j; a miss det = -1e5, tbox = the row's box, src = -1.
 *   floor:     det = best, tbox = the detection's box, src = j only when there is a hit and best > floor in f64 (false for any
 *              NaN); else det = floor, tbox = the row's box, src = -1.
 *
 * Series step, per tubelet, over its present boxes in frame order addressed by ORDINAL (position in that list), not by frame:
 * a hole inside a tubelet is no list element.  With `complete`, runs of det <= -10 are filled -- from the first / last valid
 * value at the ends, inside by l + (r-l)*(k-i+1)/(j-i+1) on ordinals; a NaN is neither missing nor filled.  A tubelet without
 * any valid value latches VDET_EINDEX (reported by vdet_sync), its det keeps the sentinels and its pooled stays NaN.  Then the
 * centred max-pool of `window` (odd; 1: a copy) over ordinals, -1e5 outside the list, writes d_pooled: starting from the
 * centre, a neighbour replaces the running value when it compares greater, so a NaN centre stays and a NaN neighbour is
 * skipped.  With complete, the filled values are also written to d_det.
 *
 * On tubelets without holes, no floor and complete = 1, det / pooled / tboxes are bit for bit vdet_rescore_tracks' and
 * vdet_video_batch's.  Per video the bits of the batch are those of the single call on that video alone.
 *
 * Host side: the regular-frame flags and the x-sorted index over the concatenated volume are those of the graph build of the
 * same boxes when the cache holds them, else rebuilt (the cached graph and lists are then dropped), exactly as
 * vdet_rescore_tracks does; VDET_NO_INDEX / VDET_FORCE_GENERAL scan whole frames instead, same results.  More than one video
 * reads the per-video table of the anchor route's batch forms, staged keyed by the offsets.  Three launches (two without a
 * video of more than 1536 frames), no host wait in asynchronous mode, inputs never modified.  The series stage keeps 11 bytes of
 * LDS per frame of the call's longest video up to 1536 frames; longer videos take a one-thread-per-series kernel.  d_boxes must
 * be 16-byte aligned.  T = 0 writes nothing.  Limits: the table at the top of this file.
 */
int vdet_rescore_tubelets(vdet_ctx *ctx, int64_t F, int64_t B, int64_t C, int T, const float *d_tracks, const int32_t *d_ntracks,
                          const float *d_boxes, const float *d_scores, const void *d_floor, int floor_f64, double overlap_thres,
                          int complete, int window, double *d_det, double *d_pooled, float *d_tboxes, int32_t *d_src);

int vdet_rescore_tubelets_batch(vdet_ctx *ctx, const int64_t *h_frame_off, int64_t V, int64_t B, int64_t C, int T,
                                const float *d_tracks, const int32_t *d_ntracks, const float *d_boxes, const float *d_scores,
                                const void *d_floor, int floor_f64, double overlap_thres, int complete, int window, double *d_det,
                                double *d_pooled, float *d_tboxes, int32_t *d_src);

/* ---- R-CNN windows on the device: the patches the CNN scorers read ----------------------------------------------------------
 *
 * rcnn_img_crop + im_transform (utils/common.py:208-280) for every box of a call in one launch: what googlenet_features
 * (vdet/image_det.py:75-106) does one box at a time on the host in front of rcnn_scoring, rcnn_sampling_scoring and
 * rcnn_sampling_dets_scoring (vdet/tubelet_cls.py:102-260).  The net itself is the caller's.  All pointers are DEVICE pointers.
 *
 * d_images [Fi,H,W,3] uint8, channel order as stored (cv2.imread gives BGR and the reference never swaps it).  A box is
 * (x1,y1,x2,y2), 1-based inclusive, f64 when boxes_f64 else f32 (widened to f64 first).  Everything up to the final cast is
 * f64, one operation per product and sum (no fused multiply-add).
 *
 * Geometry per window (S = crop_size), rcnn_img_crop line for line.  bbox = box - 1.  If padding > 0 or mode is
 * VDET_PATCH_SQUARE: scale = S / (S - 2*padding); half sizes (x2-x1+1)/2, (y2-y1+1)/2; centre = corner + half size; 'square'
 * sets both half sizes to the larger; the four corners centre -+ half*scale are rounded with Python 2's round (half AWAY from
 * zero, C round()); unclipped_w/h = x2-x1+1 / y2-y1+1; pad_x1 = max(0,-x1), pad_y1 = max(0,-y1); the corners are clipped to
 * [0, W-1] x [0, H-1]; clipped_w/h likewise; scale_x = S/unclipped_w, scale_y = S/unclipped_h; crop_w = int(round(clipped_w *
 * scale_x)), crop_h alike, pad_w = int(round(pad_x1*scale_x)), pad_h alike; if pad_h + crop_h > S then crop_h = S - pad_h, the
 * same for the width.  Otherwise (VDET_PATCH_WARP with padding 0) the corners are truncated towards zero, crop_w = crop_h = S
 * and the pads are 0.
 *
 * Resize of the clipped window (src_w x src_h) to crop_w x crop_h, bilinear, OpenCV's generic INTER_LINEAR path for 64-bit
 * input as this project fixes it: per destination column fx = (float)((dx + 0.5) * (src_w / (double)crop_w) - 0.5), sx =
 * floor(fx), fx -= sx in f32; sx < 0 -> sx = 0, fx = 0; sx >= src_w - 1 -> sx = src_w - 1, fx = 0; weights a0 = 1.f - fx and
 * a1 = fx in f32, widened; rows likewise (b0, b1).  value = (S[y0][sx]*a0 + S[y0][sx+1]*a1)*b0 + (S[y1][sx]*a0 + S[y1][sx+1]*a1)
 * *b1.  Parity of this rule with cv2.resize is UNPINNED (no OpenCV where the goldens are made); the device is bit for bit the
 * numpy statement of the rule in tests/patch_spec.py.
 *
 * Output: d_patches [M,3,S,S] in out_dtype; element [ch][pad_h + y][pad_w + x] = (float)(value - d_mean[ch]) (d_mean [3] f64
 * or NULL: (float)value), every other element 0.  VDET_PATCH_F16 / VDET_PATCH_BF16 round that f32 once, to nearest even.
 * d_patches must be 16-byte aligned.
 *
 * Status: d_ok [M] uint8, 1 for a patch the reference would have produced.  0 -- the patch is all zeros and no pixel is read --
 * when a coordinate (or a padded corner) is NaN or infinite, unclipped_w/h < 1, clipped_w/h < 1, crop_w/h < 1, the image index
 * is outside 0..Fi-1, or a VDET_PATCH_WARP window with padding 0 does not lie inside the image with x1 <= x2 and y1 <= y2 (the
 * reference raises inside cv2.resize for these, or lets numpy slice a shorter / wrapped window).
 *
 * vdet_rcnn_patches: d_boxes [N,4]; d_image_idx [N] int32 or NULL (image 0).  d_offsets [N,num,4] f64 or NULL (num = 0) is
 * sampling_boxes (vdet/tubelet_cls.py:136-142, return_orig) with the caller's draw: M = N*(num+1), window (n,0) is box n,
 * window (n,1+j) is box + d_offsets[n,j]*[w,h,w,h] with w = x2-x1, h = y2-y1 (no +1), in f64; d_sboxes [N,num+1,4] f64 or NULL
 * receives the boxes used.
 *
 * vdet_tubelet_patches: d_tracks [C,T,F,ld] (ld >= 4 elements per row: tracks, tboxes), d_ntracks [C]; frames f0 <= f < f1,
 * d_images holds Fi = f1 - f0 frames, image f - f0 is frame f.  A slot is PRESENT when t < d_ntracks[c] and column 0 of its row
 * is not NaN.  The present slots get their ordinal in the order ((f-f0)*C + c)*T + t -- frames outer, tubelets inner, the order
 * of the reference's frame loop.  d_slot [cap,3] int32 rows (c,t,f), -1 behind the count; d_count [1] int32, the TRUE number of
 * present slots even beyond cap, in which case VDET_ECAP is latched (vdet_sync) and the first cap windows are valid.  Window i
 * of d_patches [cap,3,S,S] / d_ok [cap] is slot i's box; behind the count zeros / 0.
 *
 * One launch (two for the tubelet form), on the context's stream, no host wait, inputs never modified; timed under "other".
 * ctx NULL: VDET_EINVAL, nothing touched.  Limits: 1 <= S <= 1024, S - 2*padding >= 1, H, W <= 32767, num <= 255 (the table at
 * the top of this file).
 */
#define VDET_PATCH_WARP 0
#define VDET_PATCH_SQUARE 1
#define VDET_PATCH_F32 0
#define VDET_PATCH_F16 1
#define VDET_PATCH_BF16 2

int vdet_rcnn_patches(vdet_ctx *ctx, const uint8_t *d_images, int64_t Fi, int64_t H, int64_t W, const void *d_boxes, int boxes_f64,
                      int64_t N, const int32_t *d_image_idx, const double *d_offsets, int num, const double *d_mean, int S,
                      int padding, int mode, int out_dtype, void *d_patches, uint8_t *d_ok, double *d_sboxes);

int vdet_tubelet_patches(vdet_ctx *ctx, const uint8_t *d_images, int64_t Fi, int64_t H, int64_t W, const void *d_tracks,
                         int tracks_f64, int64_t C, int T, int64_t F, int ld, const int32_t *d_ntracks, int64_t f0, int64_t f1,
                         int64_t cap, const double *d_mean, int S, int padding, int mode, int out_dtype, void *d_patches,
                         uint8_t *d_ok, int32_t *d_slot, int32_t *d_count);

/* ---- RoI pooling on the device: the Fast R-CNN route ----------------------------------------------------------------------------
 *
 * The front half of fast_rcnn_cls (vdet/tubelet_cls.py:53-76) and fast_rcnn_det (vdet/image_det.py:22-33): the backbone runs
 * once per frame and every box of the frame is pooled out of its feature map, one launch for all RoIs of a call.  BOTH rules
 * below are restated from public code that was not at hand (Caffe's ROIPoolingLayer forward with Dtype = float; the RoIAlign
 * forward of He et al. 2017 as the common detection libraries ship it) and could not be checked against it: the device is bit
 * for bit the numpy statement in tests/roipool_spec.py, which is the definition.
 *
 * d_features [Fi,K,Hf,Wf], contiguous, feat_dtype VDET_FEAT_F32 / _F16 / _BF16 (16-bit features are widened to f32 exactly);
 * boxes as they are (no 1-based shift).  A RoI is r = (float)((double)box * box_scale) per coordinate; s = (float)spatial_scale.
 * Everything below is float32, every product and sum a separate operation.
 *
 * VDET_ROI_MAX.  x1c = round(r_x1 * s) (C round(): halves away from zero), y1c, x2c, y2c alike; rw = max(x2c - x1c + 1, 1), rh
 * alike; bw = (float)rw / (float)pw, bh alike.  Bin (p,q) spans rows floor((float)p * bh) .. ceil((float)(p+1) * bh) and columns
 * alike from q and bw, each shifted by y1c / x1c and clamped to [0, Hf] / [0, Wf].  A bin with end <= start on either axis is
 * 0.  Otherwise best = -FLT_MAX and the cells, visited row-major, replace best iff v > best: NaN and -inf never win.
 *
 * VDET_ROI_ALIGN, sampling in 1 .. 8 samples per bin and axis (a fixed grid), off = aligned ? 0.5 : 0.  sx = r_x1 * s - off;
 * rw = r_x2 * s - off - sx, raised to 1 when not aligned; bw = rw / (float)pw; y alike.  Sample (iy,ix) of bin (p,q) lies at
 * y = sy + (float)p * bh + ((float)iy + 0.5f) * bh / (float)sampling, x alike.  A sample with y < -1, y > Hf, x < -1 or x > Wf
 * contributes 0.  Otherwise y <= 0 becomes 0, lo = (int)y, hi = lo + 1; if lo >= Hf - 1 then lo = hi = Hf - 1 and y = lo;
 * ly = y - lo, hy = 1 - ly; x alike; value = ((hy*hx*v[lo,lo] + hy*lx*v[lo,hi]) + ly*hx*v[hi,lo]) + ly*lx*v[hi,hi] (row, column).
 * The samples are summed iy-major, then ix, from 0, and the sum is divided by (float)(sampling*sampling) once.
 *
 * Output: d_pooled [N,K,ph,pw] in feat_dtype, the f32 value rounded once to nearest even (-FLT_MAX becomes -inf in the 16-bit
 * types).  d_ok [N] uint8: 0 -- and an all-zero block, no feature read -- when a coordinate of r is not finite, |r * s| > 2^24,
 * or the image index is outside 0..Fi-1.  A RoI wholly off the map is ok with an all-zero block.
 *
 * vdet_roi_pool: d_boxes [N,4] f32 / f64, d_image_idx [N] int32 or NULL (image 0).
 * vdet_tubelet_rois: d_tracks, d_ntracks, f0, f1, cap, d_slot, d_count exactly as vdet_tubelet_patches (the same compaction
 * kernel and the same VDET_ECAP latch); d_features holds Fi = f1 - f0 maps, map f - f0 is frame f; block i of d_pooled
 * [cap,K,ph,pw] / d_ok [cap] is slot i's box, behind the count zeros / 0.
 *
 * One launch (two for the tubelet form), on the context's stream, no host wait, inputs never modified; timed under "other".
 * ctx NULL: VDET_EINVAL, nothing touched.  Not provided: backward / argmax, the adaptive RoIAlign grid, position-sensitive
 * pooling, channels-last features.
 */
#define VDET_ROI_MAX 0
#define VDET_ROI_ALIGN 1

int vdet_roi_pool(vdet_ctx *ctx, const void *d_features, int feat_dtype, int64_t Fi, int64_t K, int64_t Hf, int64_t Wf,
                  const void *d_boxes, int boxes_f64, int64_t N, const int32_t *d_image_idx, double spatial_scale, int ph, int pw,
                  double box_scale, int mode, int sampling, int aligned, void *d_pooled, uint8_t *d_ok);

int vdet_tubelet_rois(vdet_ctx *ctx, const void *d_features, int feat_dtype, int64_t Fi, int64_t K, int64_t Hf, int64_t Wf,
                      const void *d_tracks, int tracks_f64, int64_t C, int T, int64_t F, int ld, const int32_t *d_ntracks, int64_t f0,
                      int64_t f1, int64_t cap, double spatial_scale, int ph, int pw, double box_scale, int mode, int sampling,
                      int aligned, void *d_pooled, uint8_t *d_ok, int32_t *d_slot, int32_t *d_count);

/*
 * The SVM head of the CNN scorers on the device: rcnn_scoring / rcnn_sampling_scoring (vdet/tubelet_cls.py:102-194) AFTER the
 * net -- svm_scores (vdet/image_det.py:109-114) for the one class column a window needs, the max and argmax over the windows
 * of a box (:166-189) and the scatter into the [C,T,F] layout the other stages read.
 *
 * d_feat [N*G, K]: the net's features, window m = g*G + j is window j of group (box) g, G = num + 1 windows per box;
 * feat_dtype VDET_FEAT_F32 / _F16 / _BF16 / _F64.  d_W [K,M] and d_B [M] (or NULL: no bias) as the model stores them, f64
 * when w_f64 / b_f64 else f32.  scale = 20 / feat_norm_mean, worked out by the caller.  The compute type is f64 when
 * compute_f64, else f32 -- numpy's result type: f32 only when features, W and B are all at most f32 (VDET_EINVAL otherwise).
 *
 *     s[m] = sum_k (feat[m,k] * scale) * W[k, col] + B[col]
 *
 * feat is widened to the compute type exactly, feat*scale is rounded once (the reference's order, :112-113), then every
 * product and every sum is one rounded operation (no fused multiply-add).  THE ORDER OF THE SUM: k is cut into units of 8;
 * unit u = k/8 belongs to lane u % 64; a lane adds its products to one accumulator from +0 in ascending k; the 64 accumulators
 * are combined by the butterfly acc[l] = acc[l] + acc[l ^ d] for d = 32, 16, 8, 4, 2, 1; B[col] is added last.  The order does
 * not depend on N, G, the launch or feat_dtype; tests/svm_spec.py states it in numpy and the device equals it bit for bit.
 *
 * Column: with d_slot [N,3] int32 rows (c,t,f) (vdet_tubelet_patches' d_slot), col = d_cols[c] (d_cols [C] int32; NULL: col =
 * c); without d_slot every group is class c = 0 (C must be 1, d_cols [1] or NULL).  d_count [1] int32 (vdet_tubelet_patches'
 * d_count) or NULL: groups g >= min(count, N) are skipped and their slot rows are not read.
 *
 * Per group: score = max_j s[g*G + j], arg = the first j attaining it by np.argmax's rules (the first maximum wins; a NaN wins
 * at its first occurrence and the score is NaN).  Windows with d_ok[m] == 0 (d_ok [N*G] uint8 or NULL) do not compete and
 * their features are not read; a group with no window left scores NaN with arg -1 and is counted in d_nbad [1] int32.
 *
 * Outputs.  Compact: d_score [N] (compute type), d_arg_flat [N] int32 -- NaN / -1 for a skipped group.  With d_slot: d_det
 * [C,T,F] (compute type) and d_arg [C,T,F] int32 receive score / arg at (c,t,f), and d_tboxes [C,T,F,4] f64 the winning row of
 * d_sboxes [N,G,4] f64 (vdet_rcnn_patches' d_sboxes; NaN for a group without a window); ONLY the slots of the call's groups are
 * written, so consecutive calls over the frame ranges of a video fill the same tensors.  Without d_slot d_det / d_arg are not
 * used and d_tboxes is compact, [N,4].  d_det, d_arg, d_tboxes may be NULL; d_tboxes is written only with d_sboxes.
 *
 * A slot row outside (C,T,F) or a column outside 0..M-1 in front of the count: the group is skipped (compact NaN / -1, nothing
 * else written) and VDET_EINVAL is latched for vdet_sync.  On the context's stream, no host wait: a W^T copy (a column becomes
 * contiguous), the head itself in ONE launch, and the sum of the empty groups; timed under "other".  ctx NULL: VDET_EINVAL.
 * d_feat rows are read with 16-byte loads when K % 8 == 0 and d_feat is 16-byte aligned; any K >= 1 works.
 */
#define VDET_FEAT_F32 0
#define VDET_FEAT_F16 1
#define VDET_FEAT_BF16 2
#define VDET_FEAT_F64 3

int vdet_svm_head(vdet_ctx *ctx, const void *d_feat, int feat_dtype, int64_t N, int G, int64_t K, const void *d_W, int w_f64,
                  const void *d_B, int b_f64, int64_t M, double scale, int compute_f64, const int32_t *d_slot,
                  const int32_t *d_count, int64_t C, int T, int64_t F, const int32_t *d_cols, const double *d_sboxes,
                  const uint8_t *d_ok, void *d_det, int32_t *d_arg, double *d_tboxes, void *d_score, int32_t *d_arg_flat,
                  int32_t *d_nbad);

/* vdet_svm_scores_f64 / _f32 on DEVICE buffers: the same kernel, on the context's stream, no copies and no host wait. */
int vdet_svm_scores_dev_f64(vdet_ctx *ctx, const double *d_feat, int64_t n, int64_t k, const double *d_W, const double *d_B,
                            int64_t m, double *d_out);
int vdet_svm_scores_dev_f32(vdet_ctx *ctx, const float *d_feat, int64_t n, int64_t k, const float *d_W, const float *d_B,
                            int64_t m, float *d_out);

/* ---- device pixel tracker: tubelets that follow the PIXELS of an anchor box (the role of fcn_tracker, vdet/track.py:52-106;
 *      its MATLAB arithmetic is external, parity with it is unpinned by nature).  The rule is tests/pixtrack_spec.py --------
 *
 * d_images uint8 [F,H,W,3] in the stored channel order (BGR from cv2.imread, never swapped).  Slots as in
 * vdet_track_from_anchors: d_anchor_frames [C,T] int32 (1-based, 0 = empty slot), d_anchor_boxes [C,T,4] f32 (1-based
 * inclusive), d_anchor_scores [C,T] f32 or NULL.  All arithmetic is integer on the pixels except the confidence:
 *   luma      L = (29*c0 + 150*c1 + 77*c2 + 128) >> 8
 *   box       the anchor box truncated toward zero, minus 1: 0-based (x1,y1,x2,y2), w = x2-x1+1, h = y2-y1+1; the size never
 *             changes
 *   grid      cell k of side S samples column clamp(x1 + floor((2k+1)*w / (2S)), 0, W-1), rows likewise: point sampling, edge
 *             replication
 *   template  the S x S grid k = 0..S-1 of the anchor box on the anchor frame; fixed for both directions, never updated
 *   step      f -> g = f +- step: the region is the grid k = -R..S+R-1 of the current box on frame g; every (dy,dx) in
 *             [-R,R]^2 gets SAD = sum |Tm[i,j] - Rg[i+R+dy, j+R+dx]|; the smallest (SAD, dy*dy+dx*dx, dy, dx) wins;
 *             conf = 1.0f - (float)SAD / (float)(255*S*S); conf < (float)min_conf ends the chain; the box moves by
 *             floor((2*dx*w + S) / (2S)), floor((2*dy*h + S) / (2S)); a moved box wholly outside the image ends the chain; else
 *             the row (x1+1, y1+1, x2+1, y2+1, conf) is written
 *   chain     forward and backward from the anchor row (truncated box, 1.0); also ends at the video's end and after
 *             ceil((max_frames+1)/2) - 1 steps when max_frames > 0.  Rows not written -- beyond a chain's end, on the frames a
 *             step > 1 skips, every row of an empty slot -- are NaN
 * d_tracks [C,T,F,5] f32, d_anchors [C,T,3] f32 (frame, -1, score or 0), d_ntracks [C] int32 (1 + the last live slot of the
 * class): the bits and layout of vdet_track_from_anchors' outputs, written by the ONE launch of the call (no fill pass, no host
 * table, no host wait); timed under "other".  An anchor frame outside 0..F, or on a live slot a box that is not finite, has
 * |coordinate| > 2^20, w < 1 or h < 1 after truncation or lies wholly outside the image, is latched (VDET_EINVAL at vdet_sync);
 * its slot is written as an empty one.  Reads and writes nothing of the context's cached graph, lists, index or link memo.
 * ctx NULL: VDET_EINVAL, nothing touched.  Limits: the table at the top of this file.
 */
int vdet_track_pixels(vdet_ctx *ctx, const uint8_t *d_images, int64_t F, int64_t H, int64_t W, const int32_t *d_anchor_frames,
                      const float *d_anchor_boxes, const float *d_anchor_scores, int64_t C, int T, int S, int R, double min_conf,
                      int max_frames, int step, float *d_tracks, float *d_anchors, int32_t *d_ntracks);

/* ---- greedy tubelet generation with the pixel tracker: greedily_track_from_raw_dets (vdet/track.py:189-252) for every class of
 *      a video with vdet_track_pixels' chain as track_method.  The rule is tests/pixtrack_spec.py's greedy loop --------------
 *
 * d_images uint8 [F,H,W,3]; d_boxes [F,B,4] f32 (16-byte aligned), d_scores [F,B,C] f32 as vdet_track_volume.  Per class, up to
 * max_tracks times: the best remaining detection after the monotone cursor is the anchor (stable descending order of the
 * scores; a score < thres ends the class); its box, truncated toward zero, is followed through the pixels by vdet_track_pixels'
 * rule (S, R, min_conf, max_frames, step); every detection list of a frame the new tubelet has a row on goes through
 * track_det_nms (utils/nms.pyx:128-189) against that row at nms_thres.  Frames step skips have no row: their detections stay.
 * d_tracks [C,max_tracks,F,5] f32 rows (x1,y1,x2,y2,confidence; 1.0 on the anchor row), d_anchors [C,max_tracks,3] f32 (1-based
 * frame, box index, score: vdet_track_volume's), d_ntracks [C] int32.  The slots up to ntracks are written whole (NaN where a
 * tubelet has no box); those behind it are NOT written: the caller pre-fills d_tracks with NaN and d_anchors with zeros.
 * An anchor whose box cannot be tracked (not finite, |coordinate| > 2^20, empty after truncation, wholly outside the image)
 * takes its slot with NaN rows, suppresses nothing, and is latched (VDET_EINVAL at vdet_sync); the loop goes on.
 * Three launches per track (pick; chains, grid (C,2); eager track_det_nms of irregular frames + commit), enqueued back to back:
 * no host wait.  Timed under "track_loop".  The suppression graph and the sorted lists are the context's, reused under
 * vdet_nms_track_volume's conditions and consumed likewise; no tubelet nodes are recorded (vdet_rescore_tracks takes its
 * general path on the result).  Argument checks: vdet_nms_track_volume's and vdet_track_pixels', before any launch.
 * ctx NULL: VDET_EINVAL, nothing touched.
 */
int vdet_track_volume_pixels(vdet_ctx *ctx, const uint8_t *d_images, int64_t H, int64_t W, const float *d_boxes,
                             const float *d_scores, int64_t F, int64_t B, int64_t C, double nms_thres, double thres,
                             int max_tracks, int S, int R, double min_conf, int max_frames, int step, float *d_tracks,
                             float *d_anchors, int32_t *d_ntracks);

/* ---- the pixel tracker with a scale search: tubelet boxes that grow and shrink with the object.  The rule is
 *      tests/pixtrack_spec.py's scale search; everything it does not restate is vdet_track_pixels' (vdet_track_volume_pixels')
 *
 * scales = ns levels each side (0 .. 3), scale_step = p percent per level (1 .. 25), scale_penalty = q SAD units per level
 * (0 .. 65535).  Per step f -> g with the current box b = (x1,y1,x2,y2), w = x2-x1+1, h = y2-y1+1:
 *   levels    for l in -ns .. ns: ex = sgn(l) * floor((|l|*p*w + 100) / 200), ey likewise with h; b_l = (x1-ex, y1-ey, x2+ex,
 *             y2+ey), w_l = w + 2*ex, h_l = h + 2*ey: the centre is kept exactly.  Level 0 is always admissible; l != 0 is skipped
 *             when w_l < 1, h_l < 1, w_l > 2^21 or h_l > 2^21.  Levels that give the same box are all searched
 *   search    per admissible level the region is the grid k = -R..S+R-1 of b_l on frame g, and every (dy,dx) in [-R,R]^2 gets
 *             the SAD against the anchor's S x S template (taken once, the same for every level, never updated)
 *   winner    the smallest (SAD + |l|*q, |l|, dy*dy+dx*dx, dy, dx, l) over all admissible levels and shifts
 *   conf      1.0f - (float)SAD / (float)(255*S*S) from the winner's raw SAD; conf < (float)min_conf ends the chain
 *   move      b_l moved by floor((2*dx*w_l + S) / (2S)), floor((2*dy*h_l + S) / (2S)); the box is now w_l x h_l; a moved box
 *             wholly outside the image ends the chain; else the row (x1+1, y1+1, x2+1, y2+1, conf) is written
 * scales = 0 gives the bits of the call without the search.  Outputs, layouts, the chain ends, NaN rows, the anchor row, bad
 * anchor data (latched), timing buckets ("other"; "track_loop") and launch sequences (ONE launch; three per track, no host wait,
 * no tubelet nodes recorded) are those of vdet_track_pixels and vdet_track_volume_pixels.  Argument checks: theirs and the
 * three ranges above, before any launch.  ctx NULL: VDET_EINVAL, nothing touched.  Limits: the table at the top of this file.
 */
int vdet_track_pixels_scaled(vdet_ctx *ctx, const uint8_t *d_images, int64_t F, int64_t H, int64_t W,
                             const int32_t *d_anchor_frames, const float *d_anchor_boxes, const float *d_anchor_scores, int64_t C,
                             int T, int S, int R, double min_conf, int max_frames, int step, int scales, int scale_step,
                             int scale_penalty, float *d_tracks, float *d_anchors, int32_t *d_ntracks);

int vdet_track_volume_pixels_scaled(vdet_ctx *ctx, const uint8_t *d_images, int64_t H, int64_t W, const float *d_boxes,
                                    const float *d_scores, int64_t F, int64_t B, int64_t C, double nms_thres, double thres,
                                    int max_tracks, int S, int R, double min_conf, int max_frames, int step, int scales,
                                    int scale_step, int scale_penalty, float *d_tracks, float *d_anchors, int32_t *d_ntracks);

/* ---- box-filter sampling for the pixel tracker, from an integral image of the luma that the caller builds once per video and
 *      reuses.  The rule is tests/pixtrack_spec.py's box sampling; everything it does not restate is the point-sampling calls'
 *
 * vdet_luma_integral: d_images uint8 [F,H,W,3] -> d_integral uint32 [F,H+1,W+1],
 *   I[f, y, x] = sum of L[f, r, c] over r < y, c < x  (L: vdet_track_pixels' luma; row 0 and column 0 are zero).
 * Every element is written by the call (two launches: a scan along the rows, luma in flight, then a scan down the columns in
 * place; no luma plane is staged, no scratch of the context's is used); exact.  H*W <= 2^24, so the largest entry, 255 * 2^24,
 * fits.  The table takes 4/3 of the images' bytes.  Timed under "other".
 *
 * vdet_track_pixels_box / vdet_track_volume_pixels_box: vdet_track_pixels_scaled's / vdet_track_volume_pixels_scaled's
 * arguments with d_integral (the table of the SAME video, F, H, W the images') in the place of d_images; scales = 0 is the
 * fixed-scale chain.  A cell's value is the rounded mean of its pixels instead of one pixel.  On one axis, from the (level) box's
 * origin o, extent e (w or h), the side S, the limit N (W or H), for any integer k (template: 0..S-1, region: -R..S+R-1):
 *   edges     a = o + floor(k*e / S), b = o + floor((k+1)*e / S); a' = clamp(a, 0, N-1), b' = min(max(b, a'+1), N): a cell partly
 *             outside the image averages its inside part; a cell wholly outside, or narrower than a pixel (e < S), is the nearest
 *             single column / row
 *   value     tot = I[rb',cb'] - I[ra',cb'] - I[rb',ca'] + I[ra',ca'], area = (rb'-ra') * (cb'-ca'), (tot + (area >> 1)) / area
 * SAD, key, confidence, move, chain ends, levels, bad anchor data (latched), outputs, layouts, timing buckets and launch
 * sequences (ONE launch; three per track) are those of the calls they mirror.  With w == h == S and scales = 0 every cell is one
 * pixel: vdet_track_pixels' bits.  Argument checks: those of the calls they mirror, H*W <= 2^24 and a non-NULL d_integral, before
 * any launch.  ctx NULL: VDET_EINVAL, nothing touched.  Limits: the table at the top of this file.
 */
int vdet_luma_integral(vdet_ctx *ctx, const uint8_t *d_images, int64_t F, int64_t H, int64_t W, uint32_t *d_integral);

int vdet_track_pixels_box(vdet_ctx *ctx, const uint32_t *d_integral, int64_t F, int64_t H, int64_t W,
                          const int32_t *d_anchor_frames, const float *d_anchor_boxes, const float *d_anchor_scores, int64_t C,
                          int T, int S, int R, double min_conf, int max_frames, int step, int scales, int scale_step,
                          int scale_penalty, float *d_tracks, float *d_anchors, int32_t *d_ntracks);

int vdet_track_volume_pixels_box(vdet_ctx *ctx, const uint32_t *d_integral, int64_t H, int64_t W, const float *d_boxes,
                                 const float *d_scores, int64_t F, int64_t B, int64_t C, double nms_thres, double thres,
                                 int max_tracks, int S, int R, double min_conf, int max_frames, int step, int scales,
                                 int scale_step, int scale_penalty, float *d_tracks, float *d_anchors, int32_t *d_ntracks);

/* ---- the pixel tracker with a template update and an anchor guard: the template follows an object that turns, deforms or
 *      changes lighting, and the guard keeps it from drifting onto something else.  The rule is tests/pixtrack_adapt_spec.py;
 *      everything it does not restate is tests/pixtrack_spec.py's (luma, grid, box cells, levels, key, tie order, confidence,
 *      move, outside test, bad anchors, step, max_frames, greedy loop) ----------------------------------------------------------
 *
 * vdet_track_pixels_adaptive / vdet_track_volume_pixels_adaptive: vdet_track_pixels_box's / vdet_track_volume_pixels_box's
 * arguments with d_planes and box in the place of d_integral -- box = 0: d_planes is the images uint8 [F,H,W,3] (point
 * sampling); box = 1: the integral uint32 [F,H+1,W+1] (box sampling) -- and, after the scale settings (scales = 0 allowed),
 *   update = a (0 .. 256), the weight of the new patch in 1/256;  update_conf, drift_conf: finite.
 *   state     per chain -- per slot AND direction -- A[S,S], 8.8 fixed-point integers in 0 .. 65280, initialised to Tm0 << 8.
 *             Tm0 is the anchor's template: cells 0..S-1 of the truncated anchor box on the anchor frame, point or box sampled.
 *             The backward chain starts from Tm0 again, never from what the forward chain made of it
 *   match     a step matches against Tm = (A + 128) >> 8 (uint8) in the place of the fixed template; nothing else in the step
 *             changes
 *   patch     after a step the chain keeps (conf >= min_conf and the moved box not wholly outside), with winner (l, dy, dx):
 *             P[S,S] = cells dx .. dx+S-1 (columns) by dy .. dy+S-1 (rows) of the winner's level box b_l on frame g, before
 *             the move: the window that won
 *   guard     SAD0 = sum |Tm0 - P|, c0 = 1.0f - (float)SAD0 / (float)(255*S*S)
 *   accept    a > 0 and conf >= (float)update_conf and c0 >= (float)drift_conf (f32 compares)
 *   update    on accept, element by element: A = ((256 - a) * A + a * (P << 8) + 128) >> 8.  The largest intermediate is
 *             256 * 65280 + 128; A stays within 0 .. 65280; a = 256 makes A = P << 8 (replace every frame).  With a uint8 state
 *             a small a would stall as soon as a * |P - Tm| < 128; the 8.8 state does not
 * The rows, the confidence in column 4 (the step's conf, against the CURRENT template), the NaN pattern, anchors and ntracks
 * are laid out as in the siblings: no new output.  With a = 0, or an update_conf or drift_conf no step can reach (2.0), the bits
 * are the fixed-template call's.  Launch sequences (ONE launch; three per track, no host wait) and timing buckets ("other";
 * "track_loop") are the siblings'.  Argument checks, before any launch, VDET_EINVAL: the sibling's, 0 <= update <= 256, both
 * confidences finite, box 0 or 1 (box = 1: H*W <= 2^24).  ctx NULL: VDET_EINVAL, nothing touched.  Limits: the table at the top
 * of this file.
 */
int vdet_track_pixels_adaptive(vdet_ctx *ctx, const void *d_planes, int box, int64_t F, int64_t H, int64_t W,
                               const int32_t *d_anchor_frames, const float *d_anchor_boxes, const float *d_anchor_scores, int64_t C,
                               int T, int S, int R, double min_conf, int max_frames, int step, int scales, int scale_step,
                               int scale_penalty, int update, double update_conf, double drift_conf, float *d_tracks,
                               float *d_anchors, int32_t *d_ntracks);

int vdet_track_volume_pixels_adaptive(vdet_ctx *ctx, const void *d_planes, int box, int64_t H, int64_t W, const float *d_boxes,
                                      const float *d_scores, int64_t F, int64_t B, int64_t C, double nms_thres, double thres,
                                      int max_tracks, int S, int R, double min_conf, int max_frames, int step, int scales,
                                      int scale_step, int scale_penalty, int update, double update_conf, double drift_conf,
                                      float *d_tracks, float *d_anchors, int32_t *d_ntracks);

/* ---- motion-guided propagation of detections: a frame's confident still-image detections copied to the frames around it
 *      along the motion of their pixels, so that a frame where the detector missed the object still holds a box before NMS and
 *      before tubelets are seeded (the stage T-CNN runs).  The pixels are matched ONCE per frame pair into a dense block-motion
 *      field; every box is then a lookup in a summed table of that field.  The rule is tests/motion_spec.py ----------------------
 *
 * vdet_motion_field: d_images uint8 [F,H,W,3], block P (8, 16, 32), radius R (1 .. 16), Hb = ceil(H/P), Wb = ceil(W/P) ->
 *   d_field int16 [2,F,Hb,Wb,2]     (dx, dy) of the block's best match; direction 0 is f -> f+1, direction 1 is f -> f-1
 *   d_cost  int32 [2,F,Hb,Wb]       its SAD
 *   d_fsum  int32 [2,F,Hb+1,Wb+1,2] fsum[d,f,y,x,:] = sum of field[d,f,r,c,:] over r < y, c < x (row 0 and column 0 are zero)
 *   match     block (by,bx) of frame f against frame g = f +- 1, with L vdet_track_pixels' luma: for every (dy,dx) in [-R,R]^2
 *             SAD = sum over i,j in 0..P-1 of |L_f[cy(by*P+i), cx(bx*P+j)] - L_g[cy(by*P+i+dy), cx(bx*P+j+dx)]|, cx / cy clamped
 *             to 0..W-1 / 0..H-1 (edge replication, which also defines the partial blocks at the right and at the bottom); the
 *             smallest key (SAD, dy*dy+dx*dx, dy, dx) wins: the tracker's tie order, zero motion on flat content
 *   no pair   the frame without a partner ([0,F-1] and [1,0]) is all zero in the three outputs
 * Two launches: the matching over every frame pair in both directions (no luma plane is staged), then the table; between them
 * every element of the three outputs is written exactly once.  No fill pass, no atomics, no scratch, no host wait; nothing for
 * vdet_sync to report.  Timed under "other" (one span).  d_field must be 4-byte and d_fsum 8-byte aligned.
 *
 * vdet_motion_table: the second launch alone, d_field int16 [2,F,Hb,Wb,2] -> d_fsum as above, for a caller that edits the field
 * (zeroing the vectors of blocks whose cost is high, say) before boxes are moved along it.
 *
 * vdet_propagate_boxes: the table of a video (block P, images H x W, Hb and Wb as above) and its still-image detections --
 * d_boxes f32 [F,B,4], d_scores f32 [F,B,C], d_keep_idx int32 [F,C,kcap], d_keep_cnt int32 [F,C]: vdet_nms_tracks' still-image
 * source, layout [F,B,C] only -- -> tubelet layout with T = 2*reach*top slots:
 *   sources   the first min(top, d_keep_cnt[f,c]) entries of every keep list; entry j names box b = d_keep_idx[f,c,j], whose
 *             integer box is ib = (int)v - 1 per coordinate (toward zero, as the tracker's anchors)
 *   range     on one axis, the box X1..X2 (0-based inclusive), h = P/2, N blocks: a0 = -floor((h - X1) / P), the first block
 *             whose centre pixel P*b + h is >= X1, a1 = floor((X2 - h) / P); a1 < a0 (no centre inside, a degenerate box too):
 *             a0 = a1 = floor(floor((X1 + X2) / 2) / P); both clamped to 0..N-1, then a1 = max(a1, a0)
 *   shift     with n the blocks in the two ranges and s a component summed over them (four entries of d_fsum):
 *             floor((2*s + n) / (2*n)), the mean rounded half up
 *   walk      per direction, m = 1 .. reach: the shift of step m is read from the field of the frame the box is on, in that
 *             direction, at ib + (Sx,Sy), the shift accumulated so far; after the move a box wholly outside the image
 *             (vdet_track_pixels' test) ends the chain, as does the video's end
 *   d_tracks  f32 [C,T,F,5]  slot t = di*top + j, di enumerating delta = -reach..-1, 1..reach; on g = f + delta the row is
 *             (x1 + (float)Sx, y1 + (float)Sy, x2 + (float)Sx, y2 + (float)Sy, s_m): one f32 add to the source's own coordinate;
 *             s_0 = d_scores[f,b,c], s_m = s_{m-1} * (float)decay in f32 (decay = 1: the source's bits)
 *   d_score   f32 [C,T,F] s_m;  d_src int32 [C,T,F] b;  d_ntracks int32 [C] T
 * Rows no chain reaches -- a source frame outside the video, j >= d_keep_cnt[f,c], everything behind a chain's end -- are NaN
 * with d_src = INT32_MIN.  A d_keep_cnt outside 0..kcap, a read d_keep_idx outside 0..B-1, or a source box that is not finite or
 * has |coordinate| > 2^20 latches VDET_EINVAL (vdet_sync, a message of its own); that source writes NaN rows.  A degenerate box
 * (x2 < x1) is not bad data.  ONE launch; every output element is written exactly once by it (the NaN rows are no fill pass);
 * asynchronous, no host wait, no scratch.  Timed under "other".  The outputs feed vdet_nms_tracks (with the same still-image
 * source) and every other consumer of tubelets unchanged.
 *
 * All three: argument checks before any launch, VDET_EINVAL; ctx NULL: VDET_EINVAL, nothing touched; nothing of the context's
 * cached graph, lists, index or link memo is read or written.  Limits: the table at the top of this file.
 */
int vdet_motion_field(vdet_ctx *ctx, const uint8_t *d_images, int64_t F, int64_t H, int64_t W, int block, int radius,
                      int16_t *d_field, int32_t *d_cost, int32_t *d_fsum);

int vdet_motion_table(vdet_ctx *ctx, const int16_t *d_field, int64_t F, int64_t Hb, int64_t Wb, int32_t *d_fsum);

int vdet_propagate_boxes(vdet_ctx *ctx, const int32_t *d_fsum, int64_t F, int64_t Hb, int64_t Wb, int block, int64_t H, int64_t W,
                         int64_t B, int64_t C, const float *d_boxes, const float *d_scores, const int32_t *d_keep_idx, int64_t kcap,
                         const int32_t *d_keep_cnt, int top, int reach, double decay, float *d_tracks, float *d_score,
                         int32_t *d_src, int32_t *d_ntracks);

/* ---- multi-context suppression (csrc/context_kernels.hpp): the classes among a video's highest-ranked detection scores, and a
 *      constant off every other class's scores -- the stage T-CNN runs with the propagation, before per-frame NMS and tubelet
 *      seeding.  The reference library has no function for it; the rule is tests/context_spec.py -----------------------------
 *
 * d_scores f32 [F,B,C], class innermost, 4-byte aligned (a view may start anywhere).  h_frame_off NULL: one video, outputs
 * without the V axis, no host table; h_frame_off [V+1]: V videos along F, every step per video.
 *
 * vdet_context_classes, per video:
 *   candidates  the scores that are not NaN and -- use_score_thresh != 0 -- are > (float)score_thresh (f32 compare, as
 *               vdet_top_anchors; -inf is a candidate without a threshold); n their number
 *   rank        top >= 1: k = min(top, n).  top == 0: k = max(1, floor((double)ratio * (double)n)) clamped to n, ONE f64 product,
 *               taken on the device (n is known only there)
 *   d_thresh    f32 [V]   the k-th largest candidate by float order (-0.0 == +0.0, written as +0.0); +inf when n == 0
 *   d_n         int64 [V] n
 *   d_hits      int32 [V,C] candidates of class c that are >= thresh: every tie counts, so the result depends on no index order,
 *               grid shape or run order; all zero when n == 0
 *   d_high      uint8 [V,C] hits >= min_hits
 * A radix select over the volume as it lies, integer counts only: two full reads when the keys at or above the first digit's
 * bin of rank k fit the record scratch, three when they fit only below the second digit (uniform scores), four when they never
 * do (an all-equal volume); same results.  Scratch owned by the context: 8 KiB + 32 bytes per video, and per video 8-byte records for a 64th of
 * its scores, at least 4096 and at most 2^21 of them (16 MiB).  Asynchronous, no host wait; the batch form stages the per-video
 * table keyed by the offsets and the shape.  Timed under "track_pick".
 *
 * vdet_suppress_context: d_out[f,b,c] = d_scores[f,b,c] - (float)penalty (one f32 subtraction) where d_high[v(f),c] == 0 and the
 * score is not NaN; every other element, NaN included, is copied bit for bit.  d_out == d_scores is allowed (in place); any other
 * overlap is VDET_EINVAL.  One launch, one read and one write; asynchronous, no scratch.  Timed under "other".
 *
 * Both: argument checks before any launch, VDET_EINVAL; ctx NULL: VDET_EINVAL, nothing touched; nothing of the context's cached
 * graph, lists, index or link memo is read or written.  Limits: the table at the top of this file.
 */
int vdet_context_classes(vdet_ctx *ctx, const float *d_scores, int64_t F, int64_t B, int64_t C, double ratio, int64_t top,
                         int64_t min_hits, int use_score_thresh, double score_thresh, const int64_t *h_frame_off, int64_t V,
                         float *d_thresh, int64_t *d_n, int32_t *d_hits, uint8_t *d_high);

int vdet_suppress_context(vdet_ctx *ctx, const float *d_scores, int64_t F, int64_t B, int64_t C, const uint8_t *d_high,
                          double penalty, const int64_t *h_frame_off, int64_t V, float *d_out);

/* ---- Seq-NMS (csrc/seqnms_kernels.hpp): Han et al. 2016 on per-frame detections in the tubelet layout -- link the boxes of
 *      neighbouring frames that overlap, take the sequence with the largest score sum, re-score its boxes, suppress what they
 *      overlap in their own frames, repeat.  The reference library has no function for it; the rule is tests/seqnms_spec.py ----
 *
 * d_tracks f32 [C,R,F,5] (x1, y1, x2, y2, score), d_ntracks int32 [C], d_score [C,R,F] f32 (score_f64 == 0) or f64, or NULL:
 * column 4 scores the boxes -- what vdet_nms_tracks returns.  Per class:
 *   node      row (r, f) with r < ntracks (clamped to 0..R), x1 not NaN and a finite score; the score is taken as f64 (exact)
 *   hit       hit(a, b, t): the f32 arithmetic of nms (utils/nms.pyx:57-65: +1 areas, inter, uni = (area_a + area_b) - inter),
 *             true iff uni > 0 and (double)(inter / uni) >= t.  A zero, negative or NaN union is false: nothing raises
 *   link      node (q, f) -> node (r, f+1) iff hit(box[q,f], box[r,f+1], link_thres); neighbouring frames only
 *   round k   over the nodes still live, frames ascending: best[r,f] = s[r,f] + b, b the largest best[q,f-1] among the live q that
 *             link to (r, f) and have best[q,f-1] >= 0, ptr the lowest such q attaining it; with none best = s exactly.  (Extending
 *             only from a non-negative sum makes it the maximum-sum path for negative scores too; a zero sum extends.)  The end
 *             node is the live node with the largest best -- ties: lowest frame, then lowest slot.  The rounds stop when no node is
 *             live, when best_end < min_score, or when k == max_seqs.  The sequence is ptr followed back from the end node; its
 *             sum IS best_end (the left-to-right f64 sum; nothing is summed again).  New score of its nodes: rescore 0 best_end /
 *             len (one f64 division), rescore 1 the largest s on the path (folded left to right, m = s > m ? s : m).  Every other
 *             live node (q, f) of a path node (r, f)'s frame with hit(box[r,f], box[q,f], nms_thres) is suppressed; the path
 *             nodes become members of sequence k; both leave the live set
 *   leftover  a node still live after the rounds keeps its score
 * Outputs (slots stay where they were: no compaction, no re-ranking), S = max_seqs:
 *   d_tracks_out f32 [C,R,F,5]  members and leftovers: the input box bits and (float)new score; every other row five NaNs
 *   d_score_out  f64 [C,R,F]    the new score, NaN elsewhere
 *   d_seq_out    int32 [C,R,F]  k >= 0 member of sequence k, -1 leftover, -2 suppressed, INT32_MIN no node
 *   d_ntracks_out int32 [C]     the clamped input;   d_nseq int32 [C] sequences taken
 *   d_seq_sum f64 [C,S], d_seq_len int32 [C,S], d_seq_end int32 [C,S,2] (frame, slot); NaN, 0 and -1 behind nseq
 *   d_exhausted uint8 [C]       1 iff no node was live when the rounds ended
 * The kernels write every element of every output, whatever the inputs hold.  Launches: one that writes the outputs' initial
 * state, the live bits and the link bits (scratch of the context: C*F*R*ceil(R/32) u32 -- 123 MB for 200 x 300 x 128), then
 * ceil((max_seqs + 1) / rounds) launches of one block per (video, class) with rounds = max(1, 16384 / longest video) rounds
 * each; no host wait, no block waits for another.  Timed under "track_link" and "track_loop".
 *
 * vdet_seq_nms_batch: V videos along the frames as in vdet_nms_tracks_batch -- h_frame_off [V+1], the arrays of video v start at
 * element C*R*h_frame_off[v] (times 5 for the boxes) and are [C,R,F_v,...] there; d_ntracks, d_ntracks_out, d_nseq, d_exhausted
 * [V,C]; d_seq_sum / d_seq_len [V,C,S], d_seq_end [V,C,S,2], frames counted within the video.  Per video the bits are
 * vdet_seq_nms' on that video alone; no sequence crosses a video border.  The per-video table is the staged one of vdet_query 11.
 *
 * Both: argument checks before any launch, VDET_EINVAL, nothing touched; ctx NULL: VDET_EINVAL.  Nothing of the context's cached
 * graph, lists, index or link memo is read or written.  Limits: the table at the top of this file.
 */
int vdet_seq_nms(vdet_ctx *ctx, int64_t F, int64_t C, int R, const float *d_tracks, const int32_t *d_ntracks, const void *d_score,
                 int score_f64, double link_thres, double nms_thres, int rescore, int max_seqs, double min_score,
                 float *d_tracks_out, double *d_score_out, int32_t *d_seq_out, int32_t *d_ntracks_out, int32_t *d_nseq,
                 double *d_seq_sum, int32_t *d_seq_len, int32_t *d_seq_end, uint8_t *d_exhausted);

int vdet_seq_nms_batch(vdet_ctx *ctx, const int64_t *h_frame_off, int64_t V, int64_t C, int R, const float *d_tracks,
                       const int32_t *d_ntracks, const void *d_score, int score_f64, double link_thres, double nms_thres,
                       int rescore, int max_seqs, double min_score, float *d_tracks_out, double *d_score_out, int32_t *d_seq_out,
                       int32_t *d_ntracks_out, int32_t *d_nseq, double *d_seq_sum, int32_t *d_seq_len, int32_t *d_seq_end,
                       uint8_t *d_exhausted);

/* ---- NMS over whole tubelets by spatio-temporal overlap (tube NMS of the tubelet detectors; no counterpart in the reference) ---
 *
 * Drops the tubelets of a class that repeat a better-scored tubelet of the same class, judged over their whole extent -- the
 * stage behind tracking (vdet_track_from_anchors, vdet_track_pixels) or vdet_merge_tracks and in front of the scorers.  The rule
 * is the project's own; it is stated once more in numpy (tests/tubenms_spec.py) and the device equals that statement on bits.
 *
 * Inputs, per video and class c: d_tracks [C,T,F,5] f32, d_ntracks [C] i32 (clamped to 0..T), optionally d_tboxes [C,T,F,4] f32
 * (when given they are the boxes), optionally d_anchors [C,T,3] f32 and n_series (0..4) series [C,T,F] f64 whose DEVICE pointers
 * sit in the host array h_series.  A box exists at (c,t,f) iff t < d_ntracks[c] and d_tracks[c,t,f,0] is not NaN -- the rule of
 * every other stage; slots at or behind d_ntracks[c] are never read.  Inputs are never modified.
 *
 * 1. Tubelet score ts[t] (f64).  score_mode VDET_TUBE_SCORE_SLOT: d_score is [C,T] (f32, or f64 with score_f64), the value as
 *    given, widened.  VDET_TUBE_SCORE_MEAN: d_score is [C,T,F]; ts = the f64 sum divided by the count, the sum running in
 *    ASCENDING frame order from 0.0 over the frames where the box exists and the value is not NaN.  VDET_TUBE_SCORE_MAX: the
 *    maximum over the same frames (between -0.0 and +0.0 it is +0.0, whatever the order).  No such frame: ts = NaN.  A tubelet
 *    with no box, or with a NaN ts, is ABSENT: it is not kept, suppresses nothing and cannot be suppressed.
 * 2. Frame overlap.  For tubelets a <= b (slot numbers) and a frame where both have a box: q = the f32 overlap of the
 *    conventions at the top of this file with a as box i (+1 areas, max / min as "x >= y ? x : y", inter / (area_a + area_b -
 *    inter)).  Iff q > 0 and q <= FLT_MAX the frame contributes k = (uint32) rint(q * 2^24): the product in f32 (an exact
 *    scaling), rounded to nearest even, saturated at 2^32 - 1.  A NaN, zero, negative or infinite quotient contributes 0 and
 *    latches nothing: there is no VDET_EDIVZERO here, no reference behaviour asks for one.
 * 3. Pair sums, all integers: S[a,b] = the sum of k over the shared frames (uint64), I[a,b] = the number of shared frames,
 *    n[t] = the number of frames with a box.  The sum is an integer ON PURPOSE: it does not depend on the order of the frames,
 *    so the kernels may split them over lanes, waves and workgroups however they like -- and there are no float atomics on any
 *    result path.
 * 4. Tube overlap.  den = n[a] + n[b] - I (VDET_TUBE_NORM_UNION: the mean IoU over the temporal union, the usual spatio-temporal
 *    IoU), I (VDET_TUBE_NORM_SHARED), or min(n[a], n[b]) (VDET_TUBE_NORM_MIN: a short tubelet inside a long one overlaps fully).
 *    ovr = 0.0 if den == 0 or I < min_shared, else (double)S / ((double)den * 16777216.0): one IEEE f64 division.  ovr[b,a] =
 *    ovr[a,b]; the diagonal follows the same rule.
 * 5. Selection.  The present tubelets in descending ts (-0.0 == +0.0, equal scores by DESCENDING slot) are walked once: a live
 *    tubelet is kept, and every live tubelet behind it with ovr >= thresh is suppressed.  thresh > 1 suppresses nothing: the
 *    result is the present tubelets in score order, bit for bit.
 * 6. Outputs -- every element is written by the call's launches, no fill pass by the caller.  The kept tubelets are compacted
 *    into rank order: slot r < d_ntracks_out[c] of d_tracks_out, d_tboxes_out, d_anchors_out and d_series_out [n_series][C*T*F]
 *    (vdet_merge_tracks' layout) is a bit-for-bit copy of source slot d_src[c,r]; slots behind the count are NaN rows, NaN
 *    series and zero anchors.  d_tboxes_out / d_anchors_out: given iff the input is.  d_src [C,T] i32 (INT32_MIN behind the
 *    count), d_tscore [C,T] f64 (ts of the kept slot, NaN behind the count), d_by [C,T] i32 indexed by INPUT slot: its own index
 *    if kept, the kept slot that suppressed it, -1 if absent or at or behind d_ntracks.  d_overlaps [C,T,T] f64 or NULL (not
 *    computed): ovr of every pair of present tubelets, rows and columns of every other slot NaN.
 *
 * Four launches (tubelet scores and extents; the pair pass over tiles of 32 x 32 pairs, which leaves one bit per pair; one wave
 * per class for the selection; the gather), no host wait, scratch of the context sized on demand (V*C*T*(20 + 4*ceil(T/32))
 * bytes).  Timed under "other".  Nothing of the context's cached graph, lists, index or link memo is read or written.
 *
 * vdet_nms_tubelets_batch: V videos in vdet_video_batch's layout -- the [C,T,F,...] arrays of video v start at element
 * C*T*h_frame_off[v] (times 5 / 4 for rows / tboxes), d_ntracks, d_ntracks_out [V,C], d_anchors [V,C,T,3], a per-slot d_score,
 * d_src, d_tscore, d_by [V,C,T], d_overlaps [V,C,T,T].  Per video the bits are vdet_nms_tubelets' on that video alone.  More
 * than one video reads the per-video table staged keyed by the offsets (vdet_query 11): the same offsets again neither wait
 * nor copy.
 *
 * Both: argument checks before any launch, VDET_EINVAL, nothing touched; ctx NULL: VDET_EINVAL.  Limits: the table at the top.
 */
#define VDET_TUBE_NORM_UNION 0
#define VDET_TUBE_NORM_SHARED 1
#define VDET_TUBE_NORM_MIN 2
#define VDET_TUBE_SCORE_SLOT 0
#define VDET_TUBE_SCORE_MEAN 1
#define VDET_TUBE_SCORE_MAX 2

int vdet_nms_tubelets(vdet_ctx *ctx, int64_t F, int64_t C, int T, const float *d_tracks, const int32_t *d_ntracks,
                      const float *d_tboxes, const void *d_score, int score_f64, int score_mode, const float *d_anchors,
                      const double *const *h_series, int n_series, double thresh, int norm, int min_shared, float *d_tracks_out,
                      int32_t *d_ntracks_out, float *d_tboxes_out, float *d_anchors_out, double *d_series_out, int32_t *d_src,
                      double *d_tscore, int32_t *d_by, double *d_overlaps);

int vdet_nms_tubelets_batch(vdet_ctx *ctx, const int64_t *h_frame_off, int64_t V, int64_t C, int T, const float *d_tracks,
                            const int32_t *d_ntracks, const float *d_tboxes, const void *d_score, int score_f64, int score_mode,
                            const float *d_anchors, const double *const *h_series, int n_series, double thresh, int norm,
                            int min_shared, float *d_tracks_out, int32_t *d_ntracks_out, float *d_tboxes_out, float *d_anchors_out,
                            double *d_series_out, int32_t *d_src, double *d_tscore, int32_t *d_by, double *d_overlaps);

#ifdef __cplusplus
}
#endif
#endif /* VDET_HIP_H */
