// Re-scoring of ANY tubelet set against the detections (vdet_rescore_tubelets / _batch, include/vdet_hip.h): the array form of
// raw_dets_spatial_max_pooling (reference vdet/tubelet_cls.py:493-535) + do_score_completion (:284-303) +
// score_proto_temporal_maxpool (:386-414), and -- with a FLOOR -- of the half of rcnn_sampling_dets_scoring (:221-259) that
// follows the CNN: a box keeps its own score unless an overlapping detection scores strictly higher.
//
// What differs from track_kernels.hpp's rescore_* kernels, which serve the greedy tracker's own tubelets and stay as they are:
//   * a tubelet is the LIST of its present boxes (t < ntracks and x1 not NaN), in frame order.  Completion and the temporal
//     max-pool address that list by ORDINAL, as the reference does on its list of box dicts: a hole (NaN row) inside a tubelet
//     is not a list element, so a gap is interpolated across it and the pool's neighbours are the boxes before and after it.
//   * the spatial step reports which detection won (src) and takes an optional per-box floor.
// On tubelets without holes, no floor and completion on, det / pooled / tboxes are bit for bit rescore_*'s.
//
// Layout (video_batch's): video v holds frames [f0, f0 + F_v) of the concatenated volume; its [C,T,F_v,...] block of every
// per-box array starts at element C*T*f0 (times the row width).  ntracks is [V,C].
//
// rescore_tubelets_spatial_kernel   one WAVE per (frame, class, slot), four per workgroup, grid (ceil(Fmax*C*T/4), V); the wave
//     index is frame-major ((f*C + c)*T + t) so neighbours in dispatch order scan the same frame's x-window out of L2.  On a
//     regular frame with an x-index: the window of xwindow(), an f32 screen, then the f64 test (the scan of rescore_one_scan);
//     else the whole frame in f64.  Wave argmax by shuffles, then lane 0 applies the floor and writes det / tbox / src.
// rescore_tubelets_series_kernel    one WAVE per series, grid (ceil(C*T/waves), V), videos of at most kRescoreWaveMaxF frames.
//     Per 64-frame chunk a ballot of "present" and a popcount prefix give every present frame its ordinal; value (f64), frame
//     (u16) and miss flag (u8) go to LDS at the ordinal: 11 bytes per frame of the call's longest such video.  The fill is
//     order-free (it reads the flags and PRESENT values only, which never change); the pool reads the filled list and
//     scatters by the stored frame.  No atomics on a result path (one atomicOr on the error path).
// rescore_tubelets_series_long_kernel   videos of more than kRescoreWaveMaxF frames: one THREAD per series, same ordinal
//     semantics without a stage -- it walks the frames, skipping the holes.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "track_kernels.hpp"     // xwindow, iou_f64_pair, argmax_better, FrameIndex, box_area, kSeriesWaveMaxF
#include "batch_kernels.hpp"     // VidDesc

namespace vdet {

constexpr int kRescoreWaveMaxF = kSeriesWaveMaxF;     // longest video the one-wave-per-series kernel stages in LDS
constexpr int kRescoreBytesPerFrame = 11;             // f64 value + u16 frame + u8 miss flag

struct RescoreArgs {
    const VidDesc *vids;        // null: one video of F frames
    const float *tracks;        // [C,T,F,5]
    const int32_t *ntracks;     // [V,C]
    const float4 *boxes;        // [F,B]
    const float *scores;        // [F,B,C]
    const void *floor;          // [C,T,F] f64 / f32, or null
    int floor_f64;
    int F, B, C, T;             // F: all frames of the call
    double thres;
    int complete, window;
    double *det, *pooled;       // [C,T,F]
    float *tboxes;              // [C,T,F,4]
    int32_t *src;               // [C,T,F]
    FrameIndex ix;              // x-sorted index over the concatenated volume (xbox null: none)
    const uint32_t *group_flags;
    int *err;
};

__device__ __forceinline__ VidDesc rescore_vid(const RescoreArgs &a, int v)
{
    return a.vids ? a.vids[v] : VidDesc{0, a.F};
}

__global__ __launch_bounds__(256) void rescore_tubelets_spatial_kernel(const RescoreArgs a)
{
    const int v = blockIdx.y;
    const VidDesc vd = rescore_vid(a, v);
    const int lane = threadIdx.x & 63;
    const int64_t wv = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int C = a.C, T = a.T, B = a.B;
    if (wv >= (int64_t)vd.F * C * T) return;
    const int t = (int)(wv % T);
    const int fc = (int)(wv / T);
    const int f = fc / C, c = fc - f * C;
    const int64_t e = (int64_t)C * T * vd.f0 + ((int64_t)c * T + t) * vd.F + f;
    const int64_t g = (int64_t)vd.f0 + f;           // the frame in the concatenated volume
    const float *row = a.tracks + e * 5;
    if (t >= a.ntracks[(int64_t)v * C + c] || row[0] != row[0]) {
        if (lane == 0) {
            const double qnan = __longlong_as_double(0x7FF8000000000000ll);
            a.det[e] = qnan;
            a.src[e] = -1;
        }
        if (lane < 4) a.tboxes[e * 4 + lane] = __uint_as_float(0x7FC00000u);
        return;
    }
    const double thres = a.thres;
    const double p[4] = {(double)row[0], (double)row[1], (double)row[2], (double)row[3]};
    double bs = 0.0;
    int64_t bi = -1;
    const float wc = (row[2] - row[0]) + 1.0f;
    if (a.ix.xbox && a.group_flags && (a.group_flags[g] & kFlagRegular) && thres > 1e-6 && wc > 0.0f && wc < 3.0e38f) {
        int r0, r1;
        xwindow(a.ix, (int)g, row[0], wc, thres, r0, r1);
        // the f32 screen of rescore_one_scan: whatever the f64 test accepts on a regular frame passes it
        const float pa = ((row[2] - row[0]) + 1.0f) * ((row[3] - row[1]) + 1.0f);
        const float thr_lo = (float)thres - 1.0e-3f;
        for (int r = r0 + lane; r < r1; r += 64) {
            const float4 bb = a.ix.xbox[g * B + r];
            const float sw = (fminf(row[2], bb.z) - fmaxf(row[0], bb.x)) + 1.0f;
            const float sh = (fminf(row[3], bb.w) - fmaxf(row[1], bb.y)) + 1.0f;
            if (!(sw > 0.0f && sh > 0.0f)) continue;
            const float sinter = sw * sh;
            const float suni = (pa + box_area(bb)) - sinter;
            if (!(sinter > thr_lo * suni)) continue;
            const double q[4] = {(double)bb.x, (double)bb.y, (double)bb.z, (double)bb.w};
            if (iou_f64_pair(p, q) > thres) {
                const int64_t j = a.ix.xord[g * B + r];
                const double s = (double)a.scores[(g * B + j) * C + c];
                if (argmax_better(s, j, bs, bi)) { bs = s; bi = j; }
            }
        }
    } else
    for (int j = lane; j < B; j += 64) {
        const float4 bb = a.boxes[g * B + j];
        const double q[4] = {(double)bb.x, (double)bb.y, (double)bb.z, (double)bb.w};
        if (iou_f64_pair(p, q) > thres) {
            const double s = (double)a.scores[(g * B + j) * C + c];
            if (argmax_better(s, j, bs, bi)) { bs = s; bi = j; }
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {        // wave argmax (first index on ties, NaN rules of argmax_better)
        const double s2 = __shfl_xor(bs, d, 64);
        const long long i2 = __shfl_xor((long long)bi, d, 64);
        if (i2 >= 0 && argmax_better(s2, (int64_t)i2, bs, bi)) { bs = s2; bi = (int64_t)i2; }
    }
    if (lane == 0) {
        bool take = bi >= 0;
        double out = take ? bs : -1e5;        // no floor: the sentinel of a miss (:526-530)
        if (a.floor) {
            // the box's own score stands unless a detection scores strictly higher (:245; false for any NaN)
            const double fl = a.floor_f64 ? static_cast<const double *>(a.floor)[e] : (double)static_cast<const float *>(a.floor)[e];
            take = take && bs > fl;
            if (!take) out = fl;
        }
        float4 ob = make_float4(row[0], row[1], row[2], row[3]);
        if (take) ob = a.boxes[g * B + bi];
        a.det[e] = out;
        a.tboxes[e * 4 + 0] = ob.x; a.tboxes[e * 4 + 1] = ob.y; a.tboxes[e * 4 + 2] = ob.z; a.tboxes[e * 4 + 3] = ob.w;
        a.src[e] = take ? (int32_t)bi : -1;
    }
}

// one wave per series; `waves` of them per workgroup, each with stride_bytes of LDS (the host sizes both from the longest video
// of the call, capped at kRescoreWaveMaxF: cap frames)
__global__ __launch_bounds__(256) void rescore_tubelets_series_kernel(const RescoreArgs a, int stride_bytes, int cap)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char rescore_smem[];
    const int v = blockIdx.y;
    const VidDesc vd = rescore_vid(a, v);
    const int F = vd.F;
    if (F > cap) return;          // (a long video: rescore_tubelets_series_long_kernel)
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int waves = blockDim.x >> 6;
    const int ct = blockIdx.x * waves + w;
    if (ct >= a.C * a.T) return;
    unsigned char *base = rescore_smem + (size_t)w * stride_bytes;
    volatile double *val = reinterpret_cast<volatile double *>(base);
    volatile uint16_t *fr = reinterpret_cast<volatile uint16_t *>(base + (size_t)cap * 8);
    volatile unsigned char *miss = base + (size_t)cap * 10;
    const int c = ct / a.T, t = ct - c * a.T;
    const int64_t e0 = (int64_t)a.C * a.T * vd.f0 + (int64_t)ct * F;
    const float *tr = a.tracks + e0 * 5;
    double *s = a.det + e0;
    double *o = a.pooled + e0;
    const double qnan = __longlong_as_double(0x7FF8000000000000ll);
    const bool live = t < a.ntracks[(int64_t)v * a.C + c];
    int n = 0;
    for (int f0 = 0; f0 < F; f0 += 64) {         // compaction: present frames -> ordinals
        const int f = f0 + lane;
        bool present = false;
        double x = 0.0;
        if (f < F) {
            o[f] = qnan;
            if (live) {
                const float x1 = tr[(int64_t)f * 5];
                present = x1 == x1;
                if (present) x = s[f];
            }
        }
        const unsigned long long m = __ballot(present);
        if (present) {
            const int k = n + __popcll(m & ((1ull << lane) - 1ull));
            val[k] = x;
            fr[k] = (uint16_t)f;
            miss[k] = (x <= -10.0) ? 1 : 0;
        }
        n += __popcll(m);
    }
    if (n == 0) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (a.complete) {
        bool bad = false;
        for (int i = lane; i < n; i += 64) {           // do_score_completion, on ordinals
            if (!miss[i]) continue;
            int i0 = i, j = i + 1;
            while (i0 > 0 && miss[i0 - 1]) --i0;
            while (j < n && miss[j]) ++j;
            double x;
            if (i0 == 0) {
                if (j == n) { bad = true; continue; }
                x = val[j];
            } else if (j == n) {
                x = val[i0 - 1];
            } else {
                const double l = val[i0 - 1], r = val[j];
                x = l + (r - l) * (double)(i - i0 + 1) / (double)(j - i0 + 1);
            }
            val[i] = x;
            s[fr[i]] = x;
        }
        if (__ballot(bad)) { if (lane == 0) atomicOr(a.err, 1); return; }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    const int h = a.window / 2;
    for (int i = lane; i < n; i += 64) {           // score_proto_temporal_maxpool, on ordinals
        double m = val[i];
        for (int d = -h; d <= h; ++d) {
            const int k = i + d;
            const double x = (k < 0 || k >= n) ? -1e5 : val[k];
            m = (x > m) ? x : m;
        }
        o[fr[i]] = m;
    }
}

// the next / previous present frame of a series (F / -1: none)
__device__ __forceinline__ int rescore_next_present(const float *tr, int f, int F)
{
    while (f < F && tr[(int64_t)f * 5] != tr[(int64_t)f * 5]) ++f;
    return f;
}

__device__ __forceinline__ int rescore_prev_present(const float *tr, int f)
{
    while (f >= 0 && tr[(int64_t)f * 5] != tr[(int64_t)f * 5]) --f;
    return f;
}

// videos of more than cap = kRescoreWaveMaxF frames: one thread per series
__global__ __launch_bounds__(64) void rescore_tubelets_series_long_kernel(const RescoreArgs a, int cap)
{
    const int v = blockIdx.y;
    const VidDesc vd = rescore_vid(a, v);
    const int F = vd.F;
    if (F <= cap) return;
    const int ct = blockIdx.x * 64 + threadIdx.x;
    if (ct >= a.C * a.T) return;
    const int c = ct / a.T, t = ct - c * a.T;
    const int64_t e0 = (int64_t)a.C * a.T * vd.f0 + (int64_t)ct * F;
    const float *tr = a.tracks + e0 * 5;
    double *s = a.det + e0;
    double *o = a.pooled + e0;
    const double qnan = __longlong_as_double(0x7FF8000000000000ll);
    for (int f = 0; f < F; ++f) o[f] = qnan;
    if (t >= a.ntracks[(int64_t)v * a.C + c]) return;
    int f = rescore_next_present(tr, 0, F);
    if (f == F) return;
    if (a.complete) {
        bool have_l = false;
        double l = 0.0;
        while (f < F) {
            const double x = s[f];
            if (!(x <= -10.0)) {         // a score (or a NaN: neither missing nor filled)
                l = x; have_l = true;
                f = rescore_next_present(tr, f + 1, F);
                continue;
            }
            // a run of missing scores from f: count it, find the present score behind it
            int cnt = 0, g = f;
            while (g < F && s[g] <= -10.0) { ++cnt; g = rescore_next_present(tr, g + 1, F); }
            if (!have_l && g == F) { atomicOr(a.err, 1); return; }
            const double r = g < F ? s[g] : 0.0;
            int k = 1;
            for (int q = f; q < g && k <= cnt; q = rescore_next_present(tr, q + 1, F), ++k)
                s[q] = !have_l ? r : (g == F ? l : l + (r - l) * (double)k / (double)(cnt + 1));
            f = g;
        }
    }
    const int h = a.window / 2;
    for (f = rescore_next_present(tr, 0, F); f < F; f = rescore_next_present(tr, f + 1, F)) {
        double m = s[f];
        int q = f, back = 0;                 // up to h boxes back, then forward over the window in list order
        while (back < h) {
            const int q2 = rescore_prev_present(tr, q - 1);
            if (q2 < 0) break;
            q = q2; ++back;
        }
        bool edge = back < h;
        int fwd = -back;
        for (; q < F && fwd <= h; q = rescore_next_present(tr, q + 1, F), ++fwd) {
            const double x = s[q];
            m = (x > m) ? x : m;
        }
        edge = edge || fwd <= h;
        if (edge && -1e5 > m) m = -1e5;      // ordinals outside the list count as -1e5
        o[f] = m;
    }
}

}  // namespace vdet
