// Device anchor route: the second way from detections to scored tubelets (reference vdet/track.py:109-119 track_from_det,
// vdet/tubelet_cls.py:353-383 anchor_propagate), in the [C,T,F,...] layout the other device stages read.
//
// LINK.  Slot (c, t) holds one caller-supplied anchor: a 1-based frame (0: the slot is empty) and a box.  The tubelet of a
// live slot is what the built-in tracker (track_kernels.hpp) makes from that box: the anchor row is (int-truncated box, 1.0);
// from there the chain runs forward, then backward; a step scores every proposal of the next frame with link_iou (the
// current box as the "i" box), NaN IoUs are out of the running, the best one wins, ties go to the LOWEST box index; the
// chain stops when nothing is left, when the best IoU is below the threshold, at the video's end or after `reach` steps; the
// new current box is the truncated proposal, its row (truncated box, IoU).  Rows the chain does not reach are NaN.  Nothing
// depends on the class: C is a grouping axis, ntracks[c] = 1 + the last live slot of class c.
//
// Shape: ONE launch, grid (C*T, 2) -- a workgroup per chain (slot x direction).  A chain is a dependent walk over frames, so
// the parallelism is across the chains and inside a step: the workgroup scans the frame's float4 boxes coalesced, four loads
// per thread in flight, reduces (IoU, index) in each wave by shuffles, and finishes over the waves through a slot of LDS that
// is double-buffered by step parity: one barrier per frame.  Every row of a slot is written exactly once, by this launch:
// the forward block writes the anchor row and what follows it, the backward block what precedes it, each the NaN rows beyond
// the end of its chain; a dead slot's rows are all the forward block's.  The whole frame is scanned (no x-window, no link
// memo): nothing of the context's cached graph, lists, index or memo is read or written.
//
// PROPAGATE.  Slot (c, t), t < ntracks[c]: fa = int(anchors[c,t,0]); the anchor box is tracks[c,t,fa-1,:4] widened to f64
// as it is; ov = iou_f64_pair(anchor box, box) over the B boxes of frame fa; best = np.argmax(ov) (first maximum, a NaN
// counts as the maximum, the first NaN wins: argmax_better); det_score[c,t,f] = (double)scores[fa-1, best, c] on every frame
// whose track row is not NaN, NaN elsewhere.  A zero union is a NaN overlap as in numpy, no error.  Dead slots (frame 0),
// t >= ntracks[c] and a NaN anchor row: all NaN, best = -1.  One workgroup per slot, one launch, every output written by it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "track_kernels.hpp"     // link_iou, trunc4
#include "batch_kernels.hpp"     // VidDesc
#include "tubelet_kernels.hpp"   // argmax_better, iou_f64_pair

namespace vdet {

constexpr int kStBadAnchor = 128;    // an anchor frame outside 0..F (vdet_track_from_anchors) / outside 1..F on a live slot (propagation)
constexpr int kAnchorLT = 256;       // threads per chain / per slot
constexpr int kAnchorWaves = kAnchorLT / 64;

struct AnchorLinkArgs {
    const float4 *boxes;        // [F,B]
    int F, B, C, T;             // (batch: C counts the V*C (video, class) groups, F all frames)
    const VidDesc *vids;        // batch form only: the frame range of every video
    int cls;                    // batch form only: classes per video
    const int32_t *aframes;     // [C,T] 1-based, 0: empty slot
    const float *aboxes;        // [C,T,4]
    const float *ascores;       // [C,T] or null
    float link_t32;
    int reach;
    float *tracks;              // [C,T,F,5]
    float *anchors;             // [C,T,3]
    int32_t *ntracks;           // [C]
    int *status;
};

__device__ __forceinline__ void anchor_row(float *r, float4 b, float s)
{
    r[0] = b.x; r[1] = b.y; r[2] = b.z; r[3] = b.w; r[4] = s;
}

// grid (C*T, 2): blockIdx.y = 0 links forward (and owns the slot's anchor row, its anchors entry and -- slot 0 of a class --
// the class's ntracks), 1 backward.  BATCH: the slots of V videos side by side, [V,C,T]; a chain lives in its own video's
// frames (VidDesc), its rows where video_batch keeps them (video v at element C*T*5*f0 of the flat buffer); frames are
// local to the video.  The single-video instantiation is the kernel as it was.
template <bool BATCH>
__global__ __launch_bounds__(kAnchorLT) void anchor_link_kernel(const AnchorLinkArgs a)
{
    __shared__ float sv[2][kAnchorWaves];
    __shared__ int si[2][kAnchorWaves];
    __shared__ float4 sb[2][kAnchorWaves];
    __shared__ int snt;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int slot = blockIdx.x, c = slot / a.T, t = slot - c * a.T;
    const int dir = blockIdx.y == 0 ? 1 : -1;
    int F = a.F;
    const int B = a.B;
    const float4 *boxes = a.boxes;
    float *trk;
    if (BATCH) {
        const int v = c / a.cls;
        const VidDesc vd = a.vids[v];
        F = vd.F;
        boxes += (int64_t)vd.f0 * B;
        trk = a.tracks + (int64_t)a.cls * a.T * 5 * vd.f0 + (int64_t)(slot - v * a.cls * a.T) * F * 5;
    } else {
        trk = a.tracks + (int64_t)slot * F * 5;
    }
    const int fr = a.aframes[slot];
    const bool live = fr >= 1 && fr <= F;
    const int af = live ? fr - 1 : 0;
    const float qnan = __uint_as_float(0x7FC00000u);

    if (dir > 0) {
        if (tid == 0) {
            if (fr < 0 || fr > F) atomicOr(a.status, kStBadAnchor);
            a.anchors[(int64_t)slot * 3] = (float)fr;
            a.anchors[(int64_t)slot * 3 + 1] = -1.0f;
            a.anchors[(int64_t)slot * 3 + 2] = a.ascores ? a.ascores[slot] : 0.0f;
        }
        if (t == 0) {            // (block-uniform) the class's count: 1 + its last live slot
            if (tid == 0) snt = 0;
            __syncthreads();
            for (int k = tid; k < a.T; k += kAnchorLT) {
                const int fk = a.aframes[(int64_t)c * a.T + k];
                if (fk >= 1 && fk <= F) atomicMax(&snt, k + 1);
            }
            __syncthreads();
            if (tid == 0) a.ntracks[c] = snt;
        }
    }
    if (!live) {                 // every row of a dead slot is the forward block's
        if (dir > 0)
            for (int64_t i = tid; i < (int64_t)F * 5; i += kAnchorLT) trk[i] = qnan;
        return;
    }
    float4 cur = trunc4(make_float4(a.aboxes[(int64_t)slot * 4], a.aboxes[(int64_t)slot * 4 + 1], a.aboxes[(int64_t)slot * 4 + 2],
                                    a.aboxes[(int64_t)slot * 4 + 3]));
    if (dir > 0 && tid == 0) anchor_row(trk + (int64_t)af * 5, cur, 1.0f);
    int n = 0;                   // steps linked so far (block-uniform)
    for (int step = 1; step <= a.reach; ++step) {
        const int f = af + dir * step;
        if (f < 0 || f >= F) break;
        const int par = step & 1;
        const float carea = box_area(cur);
        const float4 *fb = boxes + (int64_t)f * B;
        float bv = -1.0f;
        int bi = -1;
        float4 bb = cur;
        // the plain arg-max of a thread's boxes in ascending order: a NaN never wins, the lowest index does on ties
#define ANCHOR_TRY(X, IDX) { const float v = link_iou(cur, carea, X); if (v > bv) { bv = v; bi = (IDX); bb = X; } }
        int b = tid;
        for (; b + 3 * kAnchorLT < B; b += 4 * kAnchorLT) {
            const float4 x0 = fb[b], x1 = fb[b + kAnchorLT], x2 = fb[b + 2 * kAnchorLT], x3 = fb[b + 3 * kAnchorLT];
            ANCHOR_TRY(x0, b) ANCHOR_TRY(x1, b + kAnchorLT) ANCHOR_TRY(x2, b + 2 * kAnchorLT) ANCHOR_TRY(x3, b + 3 * kAnchorLT)
        }
        for (; b < B; b += kAnchorLT) {
            const float4 x = fb[b];
            ANCHOR_TRY(x, b)
        }
#undef ANCHOR_TRY
        const int my_bi = bi;
        // (IoU, index) travel together: the result does not depend on the order of the reduction
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            const float v2 = __shfl_xor(bv, d, 64);
            const int i2 = __shfl_xor(bi, d, 64);
            if (i2 >= 0 && (bi < 0 || v2 > bv || (v2 == bv && i2 < bi))) { bv = v2; bi = i2; }
        }
        if (lane == 0) { sv[par][w] = bv; si[par][w] = bi; }
        if (bi >= 0 && my_bi == bi) sb[par][w] = bb;       // (box indices are unique: one lane)
        __syncthreads();
        float best = sv[par][0];
        int bidx = si[par][0], bw = 0;
#pragma unroll
        for (int k = 1; k < kAnchorWaves; ++k) {
            const float v2 = sv[par][k];
            const int i2 = si[par][k];
            if (i2 >= 0 && (bidx < 0 || v2 > best || (v2 == best && i2 < bidx))) { best = v2; bidx = i2; bw = k; }
        }
        if (!(bidx >= 0 && best >= a.link_t32)) break;
        cur = trunc4(sb[par][bw]);
        if (tid == 0) anchor_row(trk + (int64_t)f * 5, cur, best);
        n = step;
    }
    // the rows beyond the end of the chain
    const int64_t lo = dir > 0 ? (int64_t)(af + n + 1) * 5 : 0, hi = dir > 0 ? (int64_t)F * 5 : (int64_t)(af - n) * 5;
    for (int64_t i = lo + tid; i < hi; i += kAnchorLT) trk[i] = qnan;
}

// np.argmax(iou([p], det[0..n))) by the whole workgroup (n >= 1): every thread returns it
template <typename TB>
__device__ __forceinline__ int64_t anchor_best(const double *p, const TB *__restrict__ det, int64_t n)
{
    __shared__ double ss[kAnchorWaves];
    __shared__ long long si[kAnchorWaves];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    double bs = 0.0;
    int64_t bi = -1;
    for (int64_t j = tid; j < n; j += kAnchorLT) {
        const double q[4] = {(double)det[4 * j], (double)det[4 * j + 1], (double)det[4 * j + 2], (double)det[4 * j + 3]};
        const double ov = iou_f64_pair(p, q);
        if (argmax_better(ov, j, bs, bi)) { bs = ov; bi = j; }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const double s2 = __shfl_xor(bs, d, 64);
        const long long i2 = __shfl_xor((long long)bi, d, 64);
        if (i2 >= 0 && argmax_better(s2, i2, bs, bi)) { bs = s2; bi = i2; }
    }
    if (lane == 0) { ss[w] = bs; si[w] = bi; }
    __syncthreads();
    bs = ss[0];
    bi = si[0];
#pragma unroll
    for (int k = 1; k < kAnchorWaves; ++k)
        if (si[k] >= 0 && argmax_better(ss[k], si[k], bs, bi)) { bs = ss[k]; bi = si[k]; }
    return bi;
}

// grid C*T, one workgroup per slot.  BATCH (vids != null in spirit): slots [V,C,T], C counts the V*C groups, `cls` the
// classes per video; tracks / det_score in video_batch's flat layout, boxes / scores of the video's own frames.
template <bool BATCH>
__global__ __launch_bounds__(kAnchorLT) void anchor_propagate_kernel(const float *__restrict__ tracks, const int32_t *__restrict__ ntracks,
                                                                     const float *__restrict__ anchors, const float *__restrict__ boxes,
                                                                     const float *__restrict__ scores, int F, int B, int C, int T,
                                                                     double *__restrict__ det_score, int32_t *__restrict__ best,
                                                                     int *__restrict__ status, const VidDesc *__restrict__ vids, int cls)
{
    const int tid = threadIdx.x;
    const int slot = blockIdx.x, c = slot / T, t = slot - c * T;
    const float *trk = tracks + (int64_t)slot * F * 5;
    int cl = c, NC = C;             // the class inside its video, classes of a score row
    if (BATCH) {
        const int v = c / cls;
        const VidDesc vd = vids[v];
        F = vd.F;
        cl = c - v * cls; NC = cls;
        const int64_t sv = slot - (int64_t)v * cls * T;
        trk = tracks + (int64_t)cls * T * 5 * vd.f0 + sv * F * 5;
        det_score += (int64_t)cls * T * vd.f0 + sv * F - (int64_t)slot * F;
        boxes += (int64_t)vd.f0 * B * 4;
        scores += (int64_t)vd.f0 * B * cls;
    }
    int nt = ntracks[c];
    nt = nt < 0 ? 0 : (nt > T ? T : nt);
    const float a0 = anchors[(int64_t)slot * 3];
    const int fa = (a0 >= 1.0f && a0 < 2147483648.0f) ? (int)a0 : 0;
    bool ok = t < nt && fa >= 1 && fa <= F;
    if (t < nt && !ok && !(a0 == 0.0f) && tid == 0) atomicOr(status, kStBadAnchor);    // (frame 0: a dead slot)
    double p[4] = {0.0, 0.0, 0.0, 0.0};
    if (ok) {
        const float *r = trk + (int64_t)(fa - 1) * 5;
        ok = !(r[0] != r[0]);
#pragma unroll
        for (int k = 0; k < 4; ++k) p[k] = (double)r[k];
    }
    const double qnan = __builtin_nan("");
    double sc = qnan;
    int64_t bi = -1;
    if (ok) {                    // (block-uniform)
        bi = anchor_best<float>(p, boxes + (int64_t)(fa - 1) * B * 4, B);
        sc = (double)scores[((int64_t)(fa - 1) * B + bi) * NC + cl];
    }
    for (int f = tid; f < F; f += kAnchorLT) {
        const float r0 = trk[(int64_t)f * 5];
        det_score[(int64_t)slot * F + f] = (ok && !(r0 != r0)) ? sc : qnan;
    }
    if (tid == 0) best[slot] = (int32_t)bi;
}

// the same arg-max on host-made f64 tables (the dict-level anchor_propagate): anchor n against the detections
// group_off[g] .. group_off[g+1] of its frame slot g = group[n]; -1 for a frame slot without detections.  grid N.
__global__ __launch_bounds__(kAnchorLT) void anchor_argmax_f64_kernel(const double *__restrict__ anchor_boxes, const int32_t *__restrict__ group,
                                                                      const double *__restrict__ det_boxes,
                                                                      const int64_t *__restrict__ group_off, int64_t *__restrict__ out)
{
    const int g = group[blockIdx.x];
    const int64_t o = group_off[g], n = group_off[g + 1] - o;
    const int64_t bi = anchor_best<double>(anchor_boxes + 4 * (int64_t)blockIdx.x, det_boxes + 4 * o, n);
    if (threadIdx.x == 0) out[blockIdx.x] = bi;
}

}  // namespace vdet
