// decode_kernels.hpp -- the middle of the Fast R-CNN route on the device: the head's (scores, deltas) -> per-class boxes.
//   vdet/image_det.py  bbox_transform_inv + clip_boxes (the decode im_detect does in numpy float64 on the host)
// THE rule is tests/decode_spec.py; decode_box below repeats it operation by operation in f64 (the library is built with
// -ffp-contract=off, so every product and sum is its own rounding) and rounds to f32 once at the end.  decode_exp is the
// spec's E: a fixed sequence of f64 operations (compare, multiply, rint, subtract, add, ldexp) with the spec's constants.
// The clip is numpy's maximum(minimum(v, hi), 0) written out: a NaN stays, everything <= 0 (-0.0 too) becomes +0.0.
//
// Four kernels, ONE decode function:
//   decode_boxes_kernel     one thread per (box, class): a 16-byte delta load, a 16-byte box store, consecutive lanes on
//                           consecutive classes; a wave that lies inside one box reads its roi through a uniform address
//   det_nms_deltas_kernel   detnms_kernels.hpp's body with the decode as its box source: one wave per (frame, class) decodes
//                           its <= 128 candidates at the gather, no [F,B,K,4] tensor exists
//   tubelet_dets_kernel     one thread per compact tubelet row: score and decoded box scattered to [C,T,F]
//   dets_as_tracks_kernel   the per-class NMS outputs rewritten in the rank layout of tracknms_kernels.hpp
// Offsets are 64-bit throughout.  The only atomics are the status latch and the integer max of ntracks.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "detnms_kernels.hpp"

namespace vdet {

constexpr int kStDecodeBad = 16384;     // vdet_tubelet_dets: a slot row outside shape or a class column outside K (the row is skipped)

// tests/decode_spec.py: E_HI, E_LO, E_LOG2E, E_LN2_HI, E_LN2_LO, E_COEF
__device__ __forceinline__ double decode_exp(double x)
{
    const bool nan = x != x, hi = x > 709.0, lo = x < -708.0;
    const double xs = (nan || hi || lo) ? 0.0 : x;
    const double k = __builtin_rint(xs * 0x1.71547652b82fep+0);
    const double r = (xs - k * 0x1.62e42fee00000p-1) - k * 0x1.a39ef35793c76p-33;
    double p = 0x1.6124613a86d09p-33;       // 1/13!
    p = p * r + 0x1.1eed8eff8d898p-29;      // 1/12!
    p = p * r + 0x1.ae64567f544e4p-26;
    p = p * r + 0x1.27e4fb7789f5cp-22;
    p = p * r + 0x1.71de3a556c734p-19;
    p = p * r + 0x1.a01a01a01a01ap-16;
    p = p * r + 0x1.a01a01a01a01ap-13;
    p = p * r + 0x1.6c16c16c16c17p-10;
    p = p * r + 0x1.1111111111111p-7;
    p = p * r + 0x1.5555555555555p-5;
    p = p * r + 0x1.5555555555555p-3;
    p = p * r + 0.5;
    p = p * r + 1.0;
    p = p * r + 1.0;
    const double e = __builtin_ldexp(p, (int)k);        // exact: |k| <= 1023 and the result is a normal number
    return nan ? x : (hi ? __builtin_inf() : (lo ? 0.0 : e));
}

__device__ __forceinline__ double decode_clip(double v, double hi)
{
    return v != v ? v : (v > hi ? hi : (v > 0.0 ? v : 0.0));
}

constexpr double kDecodeEps = 1e-14;    // the width term of the Fast R-CNN decode (tests/decode_spec.py: EPS)

// the roi and the deltas in f64 (widened exactly), wmax = W - 1, hmax = H - 1, off the width term: w = (x2 - x1) + off
__device__ __forceinline__ float4 decode_box_f64(double x1, double y1, double x2, double y2, double dx, double dy, double dw, double dh,
                                                 double wmax, double hmax, double off)
{
    const double w = (x2 - x1) + off, h = (y2 - y1) + off;
    const double cx = x1 + 0.5 * w, cy = y1 + 0.5 * h;
    const double pcx = dx * w + cx, pcy = dy * h + cy;
    const double pw = decode_exp(dw) * w, ph = decode_exp(dh) * h;
    const double hw = 0.5 * pw, hh = 0.5 * ph;
    return make_float4((float)decode_clip(pcx - hw, wmax), (float)decode_clip(pcy - hh, hmax),
                       (float)decode_clip(pcx + hw, wmax), (float)decode_clip(pcy + hh, hmax));
}

// the roi widened exactly to f64, the class's deltas; off is kDecodeEps for the Fast R-CNN callers, 1.0 for the RPN's anchors
__device__ __forceinline__ float4 decode_box(double x1, double y1, double x2, double y2, float4 d, double wmax, double hmax, double off)
{
    return decode_box_f64(x1, y1, x2, y2, (double)d.x, (double)d.y, (double)d.z, (double)d.w, wmax, hmax, off);
}

// a roi row widened exactly to f64: rois [N,4] f32 (one 16-byte load) or f64 (two)
template <bool F64>
__device__ __forceinline__ void load_roi(const void *rois, int64_t nb, double (&r)[4])
{
    if (F64) {
        const double2 *q = static_cast<const double2 *>(rois) + nb * 2;
        const double2 a = q[0], b = q[1];
        r[0] = a.x; r[1] = a.y; r[2] = b.x; r[3] = b.y;
    } else {
        const float4 a = static_cast<const float4 *>(rois)[nb];
        r[0] = (double)a.x; r[1] = (double)a.y; r[2] = (double)a.z; r[3] = (double)a.w;
    }
}

struct DecodeArgs {
    const void *rois;           // [N,4] f32 or f64, 16-byte aligned
    const float4 *deltas;       // [N,K]
    int64_t N;
    int K;
    double wmax, hmax;          // W - 1, H - 1
    float4 *boxes;              // [N,K]
};

template <bool F64>
__global__ __launch_bounds__(256) void decode_boxes_kernel(const DecodeArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, total = a.N * a.K;
    const int64_t nb = (i < total ? i : total - 1) / a.K;
    // a wave whose 64 elements belong to one box reads the roi through a wave-uniform address (one scalar load)
    const int64_t nb0 = ((int64_t)__builtin_amdgcn_readfirstlane((int)(nb >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)nb);
    const bool one_box = __ballot(nb != nb0) == 0ull;
    if (i >= total) return;
    const float4 d = a.deltas[i];
    double r[4];
    if (one_box) load_roi<F64>(a.rois, nb0, r);
    else load_roi<F64>(a.rois, nb, r);
    a.boxes[i] = decode_box(r[0], r[1], r[2], r[3], d, a.wmax, a.hmax, kDecodeEps);
}

// the box source of det_nms_body: decode box id of frame f for the class slot e at the gather
template <bool F64>
struct DetBoxFromDeltas {
    const void *rois;           // [F,B,4]
    const float4 *deltas;       // [F,B,K]
    int B;
    double wmax, hmax;
    __device__ __forceinline__ float4 operator()(int64_t e, int f, int id) const
    {
        double r[4];
        load_roi<F64>(rois, (int64_t)f * B + id, r);
        return decode_box(r[0], r[1], r[2], r[3], deltas[e], wmax, hmax, kDecodeEps);
    }
};

template <bool F64>
__global__ __launch_bounds__(256) void det_nms_deltas_kernel(const DetNmsParams prm, const DetBoxFromDeltas<F64> src)
{
    det_nms_body(prm, src);
}

struct TubeletDetsArgs {
    const float *scores;        // [N,K]
    const float4 *deltas;       // [N,K]
    const void *tracks;         // [C,T,F,ld] f32 or f64, the box is the first four of a row
    int ld;
    const int32_t *slot;        // [N,3] rows (c,t,f)
    const int32_t *count;       // [1] or null: all N
    const int32_t *cols;        // [C] or null: c + 1
    int64_t N;
    int K;
    int64_t C, F;
    int T;
    double wmax, hmax;
    double *det;                // [C,T,F]
    float4 *tboxes;             // [C,T,F]
    int *status;
};

template <bool F64>
__global__ __launch_bounds__(256) void tubelet_dets_kernel(const TubeletDetsArgs a)
{
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int64_t cnt = a.N;
    if (a.count) { const int64_t c0 = a.count[0]; cnt = c0 < 0 ? 0 : (c0 < a.N ? c0 : a.N); }
    if (n >= cnt) return;
    const int c = a.slot[n * 3], t = a.slot[n * 3 + 1], f = a.slot[n * 3 + 2];
    const bool in_shape = c >= 0 && c < a.C && t >= 0 && t < a.T && f >= 0 && f < a.F;
    const int col = in_shape ? (a.cols ? a.cols[c] : c + 1) : -1;
    if (!in_shape || col < 0 || col >= a.K) {
        atomicOr(a.status, kStDecodeBad);
        return;
    }
    const int64_t o = ((int64_t)c * a.T + t) * a.F + f, e = n * a.K + col;
    double x1, y1, x2, y2;
    if (F64) {
        const double *r = static_cast<const double *>(a.tracks) + o * a.ld;
        x1 = r[0]; y1 = r[1]; x2 = r[2]; y2 = r[3];
    } else {
        const float *r = static_cast<const float *>(a.tracks) + o * a.ld;
        x1 = r[0]; y1 = r[1]; x2 = r[2]; y2 = r[3];
    }
    a.det[o] = (double)a.scores[e];
    a.tboxes[o] = decode_box(x1, y1, x2, y2, a.deltas[e], a.wmax, a.hmax, kDecodeEps);
}

struct DetsAsTracksArgs {
    const float *dets;          // [F,K,topk,5]
    const int32_t *sel_idx;     // [F,K,topk]
    const int32_t *keep;        // [F,K,topk]
    const int32_t *keep_cnt;    // [F,K]
    int64_t F;
    int K, class0, R;           // R = topk
    float *tracks;              // [C,R,F,5], C = K - class0
    double *score;              // [C,R,F]
    int32_t *src;               // [C,R,F]
    int32_t *cnt;               // [C,F]
    int32_t *ntracks;           // [C], zeroed by the host before the launch
};

// one thread per (c, r, f), f innermost: the stores of a wave are contiguous, the gathers stay inside a few lists
__global__ __launch_bounds__(256) void dets_as_tracks_kernel(const DetsAsTracksArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t C = a.K - a.class0;
    if (i >= C * a.R * a.F) return;
    const int64_t f = i % a.F, cr = i / a.F;
    const int r = (int)(cr % a.R), c = (int)(cr / a.R);
    const int64_t p = f * a.K + (c + a.class0);
    int n = a.keep_cnt[p];
    n = n < 0 ? 0 : (n < a.R ? n : a.R);
    const float nanf = __builtin_nanf("");
    float v[5] = {nanf, nanf, nanf, nanf, nanf};
    int32_t s = INT32_MIN;
    if (r < n) {
        const int row = a.keep[p * a.R + r];
        if (row >= 0 && row < a.R) {
            const float *d = a.dets + (p * a.R + row) * 5;
#pragma unroll
            for (int k = 0; k < 5; ++k) v[k] = d[k];
            s = a.sel_idx[p * a.R + row];
        }
    }
    float *o = a.tracks + i * 5;
#pragma unroll
    for (int k = 0; k < 5; ++k) o[k] = v[k];
    a.score[i] = (double)v[4];
    a.src[i] = s;
    if (r == 0) {
        a.cnt[(int64_t)c * a.F + f] = n;
        if (n > 0) atomicMax(a.ntracks + c, n);
    }
}

}  // namespace vdet
