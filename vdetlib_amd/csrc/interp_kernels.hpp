// Device form of score_proto_interpolation (reference vdet/tubelet_cls.py:416-490): tubelets that live on a SAMPLED frame axis
// (every stride-th frame of the video, or a dense axis with holes) are interpolated back to every frame of the video, all
// tubelet slots of a video -- or of a vdet_video_batch -- in ONE launch, in the [C,T,F,...] layout the other device stages read.
//
// Slot (c, t) of a video: the KNOTS are the rows i of tracks[c, t, :, :] whose column 0 is not NaN, t < ntracks[c] (the tubelet
// definition of tcn_kernels.hpp).  Row i sits at the dense 1-based frame x(i) = frames[i] (strictly ascending; no table:
// i + 1).  With L knots and F dense frames:
//   L == 0   every output of the slot is NaN;
//   L == 1   the one box is copied to its frame (the reference copies tubelets of < 2 boxes, :452-454);
//   L >= 2   dense frames lo..hi, lo / hi the first / last knot frame with the reference's end rule lo == 2 -> 1,
//            hi == F - 1 -> F (:472-475); NaN outside.
// Arithmetic = series_interp_kernel's (tubelet_kernels.hpp) / oracle.interp_linear's in f64, operation for operation, without
// contraction: the knot's own y at a knot; between two knots slope = (y[j+1]-y[j])/(x[j+1]-x[j]), slope*(x - x[j]) + y[j]
// from the LEFT knot; at frame 1 below the knots y[0] + (x - x[0])*(y[1]-y[0])/(x[1]-x[0]); at frame F above them
// y[-1] + (x - x[-1])*(y[-1]-y[-2])/(x[-1]-x[-2]).  A NaN in a knot's field flows through that arithmetic.
//
// Fields: the box (boxes[c,t,i] when given, else track columns 0-3; the f32 values widened to f64 as they are), up to 4 caller
// series (f64 or f32: each a det_score field of the reference), the anchor offset x(i) - x(int(anchors[c,t,0]) - 1) in dense
// frame units, and the track score (column 4).  The reference's interpolated boxes drop track_score; interpolating it by the
// same rule is this build's own choice (the device TCN reads it as a channel).
//
// Shape of the kernel: one wave per slot walks the sampled rows 64 at a time.  A ballot marks the chunk's knots; every knot
// lane finds its LEFT neighbour knot in the ballot mask (or takes the last knot of the earlier chunks, which the wave carries
// in scalar registers), writes its own frame and fills the dense frames between the two.  The intervals between consecutive
// knots tile lo..hi, so every dense frame is written exactly once, by the kernel, NaN included -- no knot list is kept, in
// LDS or anywhere else, and there is no limit on Fs, F or the stride.  A gap of more than kInterpLaneGap dense frames is not
// left to its one lane: the wave fills it together, 64 frames per step.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vdet {

constexpr int kInterpMaxSeries = 4;
constexpr int kInterpFields = 6 + kInterpMaxSeries;   // x1 y1 x2 y2 | track score | anchor | series
constexpr int kInterpLaneGap = 64;                     // longer gaps between two knots are filled by the whole wave

struct InterpArgs {
    const float *tracks;                  // [C,T,Fs,5] per video
    const float *boxes;                   // [C,T,Fs,4] per video, or null: the track boxes
    const int32_t *ntracks;               // [V,C]
    const float *anchors;                 // [V,C,T,3]
    const void *series[kInterpMaxSeries]; // [C,T,Fs] per video, f64 (ser_f64) or f32
    int nser;
    const int64_t *soff, *doff;           // [V+1] sampled / dense frame offsets of the videos; null: one video of Fs1 / F1
    const int32_t *frames;                // [soff[V]] dense 1-based frame of every sampled row; null: row i is frame i + 1
    int Fs1, F1, C, T;
    float *otracks;                       // [C,T,F,5]
    double *boxes64;                      // [C,T,F,4]
    float *tboxes;                        // [C,T,F,4]
    double *oseries;                      // [nser][N], N = C*T*F elements of the whole call
    int64_t N;
    double *oanchor;                      // [C,T,F]
    float *oanchors;                      // [V,C,T,3]
};

// one slot's view of the arguments
struct InterpSlot {
    int64_t sb, db;          // element base of the slot on the sampled / dense axis
    const int32_t *fr;       // the video's frame table (null: identity)
    double xa;               // dense frame of the anchor row (NaN: the anchor row is not a row of the video)
};

// (rows and frames of one video fit 31 bits: C*T*F < 2^31 on both axes)
__device__ __forceinline__ int interp_frame(const InterpSlot &s, int row) { return s.fr ? s.fr[row] : row + 1; }

template <int NSER, bool SF64>
__device__ __forceinline__ void interp_load(const InterpArgs &a, const InterpSlot &s, int row, int x, double (&y)[kInterpFields])
{
    const float *tp = a.tracks + (s.sb + row) * 5;
    const float *bp = a.boxes ? a.boxes + (s.sb + row) * 4 : tp;
#pragma unroll
    for (int k = 0; k < 4; ++k) y[k] = (double)bp[k];
    y[4] = (double)tp[4];
    y[5] = (double)x - s.xa;
#pragma unroll
    for (int q = 0; q < kInterpMaxSeries; ++q) {
        y[6 + q] = 0.0;
        if (q < NSER)
            y[6 + q] = SF64 ? static_cast<const double *>(a.series[q])[s.sb + row]
                                 : (double)static_cast<const float *>(a.series[q])[s.sb + row];
    }
}

// every output of dense frame x (1-based); the f32 forms are rounded once from the f64 values
template <int NSER>
__device__ __forceinline__ void interp_store(const InterpArgs &a, const InterpSlot &s, int x, const double (&y)[kInterpFields])
{
    const int64_t e = s.db + x - 1;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float v = (float)y[k];
        a.boxes64[e * 4 + k] = y[k];
        a.tboxes[e * 4 + k] = v;
        a.otracks[e * 5 + k] = v;
    }
    a.otracks[e * 5 + 4] = (float)y[4];
    a.oanchor[e] = y[5];
#pragma unroll
    for (int q = 0; q < kInterpMaxSeries; ++q)
        if (q < NSER) a.oseries[q * a.N + e] = y[6 + q];
}

// One job of the main loop.  The knots (row rl, frame xl) and (row rr, frame xr) are neighbours (rl < 0: rr is the
// tubelet's first knot and only its own frame is asked for); the job writes the dense frames xb + off, xb + off + step, ...
// <= xe of (xl, xr], plus frame 1 when `front` (the end rule at the first two knots).  A lane runs its own job (off 0,
// step 1), the wave runs a long one together (off = lane, step 64): the same code, one store site.
template <int NSER, bool SF64>
__device__ __forceinline__ void interp_job(const InterpArgs &a, const InterpSlot &s, int rl, int rr, int xl, int xr, int xb, int xe, bool front,
                                           int off, int step)
{
    double yl[kInterpFields], yr[kInterpFields], slope[kInterpFields];
    interp_load<NSER, SF64>(a, s, rr, xr, yr);
    if (rl >= 0) {
        interp_load<NSER, SF64>(a, s, rl, xl, yl);
    } else {
#pragma unroll
        for (int k = 0; k < kInterpFields; ++k) yl[k] = yr[k];
    }
    const double dx = (double)xr - (double)xl;
#pragma unroll
    for (int k = 0; k < kInterpFields; ++k) slope[k] = (yr[k] - yl[k]) / dx;
    const int64_t n = (int64_t)xe - xb + 1;
    for (int64_t i = off; i < n + (front ? 1 : 0); i += step) {
        const int x = i < n ? xb + (int)i : 1;
        const double d = (double)x - (double)xl;
        double r[kInterpFields];
#pragma unroll
        for (int k = 0; k < kInterpFields; ++k)
            r[k] = x == xr ? yr[k] : (x < xl ? yl[k] + d * (yr[k] - yl[k]) / dx : slope[k] * d + yl[k]);
        interp_store<NSER>(a, s, x, r);
    }
}

// grid (C*T, V), one wave per slot; NSER series of f64 (SF64) or f32 values
template <int NSER, bool SF64>
__global__ __launch_bounds__(64) void interp_tracks_kernel(InterpArgs a)
{
    const int lane = threadIdx.x;
    const int v = blockIdx.y;
    const int ct = blockIdx.x, c = ct / a.T, t = ct - c * a.T;
    const int64_t s0 = a.soff ? a.soff[v] : 0, d0 = a.doff ? a.doff[v] : 0;
    const int Fs = a.soff ? (int)(a.soff[v + 1] - s0) : a.Fs1, F = a.doff ? (int)(a.doff[v + 1] - d0) : a.F1;
    const int64_t tub = (int64_t)v * a.C * a.T + ct;
    InterpSlot s;
    s.sb = (int64_t)a.C * a.T * s0 + (int64_t)ct * Fs;
    s.db = (int64_t)a.C * a.T * d0 + (int64_t)ct * F;
    s.fr = a.frames ? a.frames + s0 : nullptr;
    int nt = a.ntracks[(int64_t)v * a.C + c];
    nt = nt < 0 ? 0 : (nt > a.T ? a.T : nt);
    const bool live = t < nt;
    const double qnan = __builtin_nan("");
    // the anchor: int(anchors[c, t, 0]) is a 1-based row of the sampled axis; column 0 of the output names its dense frame
    const float a0 = a.anchors[tub * 3];
    const int arow = (a0 >= 1.0f && a0 < 2147483648.0f) ? (int)a0 - 1 : -1;
    const bool aok = live && arow >= 0 && arow < Fs;
    s.xa = aok ? (double)interp_frame(s, arow) : qnan;
    if (lane == 0) {
        a.oanchors[tub * 3] = aok ? (float)s.xa : a0;
        a.oanchors[tub * 3 + 1] = a.anchors[tub * 3 + 1];
        a.oanchors[tub * 3 + 2] = a.anchors[tub * 3 + 2];
    }
    int first = -1, last = -1, last2 = -1;     // rows of the first, the last and the last but one knot so far (wave-uniform)
    int L = 0;
    for (int64_t fb64 = 0; live && fb64 < Fs; fb64 += 64) {
        const int fb = (int)fb64, row = fb + lane;
        bool has = false;
        if (row < Fs) {
            const float r0 = a.tracks[(s.sb + row) * 5];
            has = !(r0 != r0);
        }
        const unsigned long long m = __ballot(has);
        if (m == 0) continue;
        const unsigned long long below = m & ((1ull << lane) - 1ull);
        const int prev = below ? fb + (63 - __clzll((long long)below)) : last;     // the left neighbour knot (-1: none)
        const int j = L + __popcll(below);                                            // this knot's position in the tubelet
        int x = 0, xl = 0;
        if (has) {
            x = interp_frame(s, row);
            xl = prev >= 0 ? interp_frame(s, prev) : x - 1;
        }
        // the lane's own job: its knot and the frames behind the left neighbour -- unless they are more than kInterpLaneGap:
        // then the lane keeps the knot (and frame 1), and the wave fills the interval together, one such interval at a time
        const bool wide = has && x - xl - 1 > kInterpLaneGap;
        unsigned long long w = __ballot(wide);
        bool act = has, front = has && j == 1 && xl == 2;
        int rl = prev, rr = row, jxl = xl, jxr = x, xb = wide ? x : xl + 1, xe = x, off = 0, step = 1;
        for (;;) {
            if (act) interp_job<NSER, SF64>(a, s, rl, rr, jxl, jxr, xb, xe, front, off, step);
            if (!w) break;
            const int src = __ffsll((long long)w) - 1;
            w &= w - 1;
            rl = __shfl(prev, src);
            rr = fb + src;
            jxl = __shfl(xl, src);
            jxr = __shfl(x, src);
            xb = jxl + 1; xe = jxr - 1;
            act = true; front = false; off = lane; step = 64;
        }
        const int top = 63 - __clzll((long long)m);
        const unsigned long long rest = m & ~(1ull << top);
        if (first < 0) first = fb + (__ffsll((long long)m) - 1);
        last2 = rest ? fb + (63 - __clzll((long long)rest)) : last;
        last = fb + top;
        L += __popcll(m);
    }
    // the frames outside lo..hi are NaN; the end rule at the back (frame F from the last two knots) is one of them
    int lo = F + 1, hi = F;                    // L == 0: NaN everywhere
    bool back = false;
    if (L > 0) {
        lo = interp_frame(s, first);
        hi = interp_frame(s, last);
        if (L >= 2 && lo == 2) lo = 1;
        back = L >= 2 && hi == F - 1;
    }
    for (int64_t i = lane; i < (int64_t)(lo - 1) + (F - hi); i += 64) {
        const int x = i < lo - 1 ? 1 + (int)i : hi + 1 + (int)(i - (lo - 1));
        double r[kInterpFields];
#pragma unroll
        for (int k = 0; k < kInterpFields; ++k) r[k] = qnan;
        if (back && x == F) {
            const int x0 = interp_frame(s, last2);
            double y0[kInterpFields], y1[kInterpFields];
            interp_load<NSER, SF64>(a, s, last2, x0, y0);
            interp_load<NSER, SF64>(a, s, last, hi, y1);
            const double dx = (double)hi - (double)x0, d = (double)F - (double)hi;
#pragma unroll
            for (int k = 0; k < kInterpFields; ++k) r[k] = y1[k] + d * (y1[k] - y0[k]) / dx;
        }
        interp_store<NSER>(a, s, x, r);
    }
}

}  // namespace vdet
