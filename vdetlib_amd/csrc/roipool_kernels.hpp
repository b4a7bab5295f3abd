// RoI pooling on the device (vdet_roi_pool / vdet_tubelet_rois, include/vdet_hip.h): the front half of the Fast R-CNN route --
// every box of a call pooled out of the backbone's feature map in one launch.  Two rules, both restated from public code that
// was not at hand; tests/roipool_spec.py states the same float32 arithmetic in numpy and the two are compared
// bit for bit.  Every product and sum is a separate operation (the library is built with -ffp-contract=off).
//
// roi_pool_kernel<FeatT, ALIGN, WPC>   one WORKGROUP of 256 per (RoI, chunk of the RoI's [K,ph,pw] output span), on a 1-D
//     grid.  The block index fixes the RoI, so its box, slot row and image index are uniform loads.  The RoI's geometry is
//     computed ONCE per workgroup into a small LDS table, by the first lanes, one table entry each: for 'max' the ph row
//     bins' and pw column bins' [start, end) cells (f32 edges, shifted, clamped); for 'align' the ph*sampling row samples'
//     and pw*sampling column samples' (lo, hi, l, h), lo = -1 for a sample off the map.  After one barrier the lanes take
//     the chunk's elements in one of two orders, both measured:
//       WPC (a wave per channel)  the chunk is kRoiWaveCh channels, wave w takes channels w, w + 4, ..., its lanes the bins
//           b = lane, lane + 64, ...: a wave reads ONE feature plane and writes the channel's ph*pw elements as one run;
//       span                      the chunk is kRoiChunk consecutive elements, lane i takes e = start + i, + 256, ...: every
//           store instruction is a run of 64 elements, a wave may straddle two channels.
//     Either way consecutive lanes hold consecutive bins q of a row -- adjacent column ranges of the same feature row -- and
//     write consecutive elements of the span.  A RoI that is not ok gets zeros.  Offsets into the features and the output
//     are 64-bit.  No atomics.  The host picks the order per mode (roi_launch in vdet_capi.hip); VDET_ROIPOOL_ORDER = 1 / 2
//     forces span / WPC for every mode, so that the comparison can be repeated.
#pragma once

#include <float.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "patch_kernels.hpp"

namespace vdet {

constexpr int kRoiMaxPooled = 32;     // ph, pw
constexpr int kRoiMaxSampling = 8;    // 'align' samples per bin and axis
constexpr int kRoiMaxHW = 32767;      // Hf, Wf
constexpr int kRoiChunk = 4096;       // output elements per workgroup
constexpr int kRoiWaveCh = 64;        // channels per workgroup of the wave-per-channel order
constexpr int kRoiTab = kRoiMaxPooled * kRoiMaxSampling;     // table entries per axis

struct RoiArgs {
    const void *features;       // [Fi,K,Hf,Wf] FeatT
    int Fi, Hf, Wf;
    int64_t K;
    const void *boxes;          // rows of ld elements, f32 or f64; columns 0..3 are x1,y1,x2,y2
    int boxes_f64, ld;
    const int32_t *image_idx;   // [N] or null (image 0)           -- array form
    const int32_t *slot;        // [N,3] (c,t,f) or null           -- tubelet form: box = row ((c*T + t)*F + f), image f - f0
    int T;
    int64_t F, f0;
    double box_scale;
    float spatial_scale;
    int ph, pw, sampling, aligned;
    int64_t N, span;            // RoIs; K*ph*pw
    int nchunks;                // workgroups per RoI
    void *pooled;               // [N,K,ph,pw] FeatT
    uint8_t *ok;                // [N]
};

template <typename FeatT> __device__ __forceinline__ float roi_widen(FeatT v);
template <> __device__ __forceinline__ float roi_widen<float>(float v) { return v; }
template <> __device__ __forceinline__ float roi_widen<_Float16>(_Float16 v) { return (float)v; }
template <> __device__ __forceinline__ float roi_widen<PatchBf16>(PatchBf16 v) { return __uint_as_float((uint32_t)v.u << 16); }

// one axis of 'align': sample j = p*sampling + i of a RoI that starts at s with bins of b.  lo = -1: the sample is off the map
__device__ __forceinline__ void roi_align_sample(int j, int sampling, float s, float b, int size, int &lo, int &hi, float &l, float &h)
{
    const int p = j / sampling, i = j - p * sampling;
    float y = s + (float)p * b + ((float)i + 0.5f) * b / (float)sampling;
    lo = -1; hi = 0; l = 0.f; h = 0.f;
    if (y < -1.0f || y > (float)size) return;
    if (y <= 0.f) y = 0.f;
    lo = (int)y;
    if (lo >= size - 1) {
        lo = hi = size - 1;
        y = (float)lo;
    } else {
        hi = lo + 1;
    }
    l = y - (float)lo;
    h = 1.0f - l;
}

template <typename FeatT, bool ALIGN, bool WPC>
__global__ __launch_bounds__(256) void roi_pool_kernel(const RoiArgs a)
{
    __shared__ int s_lo[2][kRoiTab], s_hi[2][kRoiTab];      // [0]: rows, [1]: columns
    __shared__ float s_l[2][ALIGN ? kRoiTab : 1], s_h[2][ALIGN ? kRoiTab : 1];
    const int64_t n = blockIdx.x / (unsigned)a.nchunks;
    const int chunk = (int)(blockIdx.x - n * a.nchunks);
    // the RoI's box and image: the same for every lane
    int64_t row = -1, img = 0;
    if (a.slot) {
        const int c = a.slot[n * 3], t = a.slot[n * 3 + 1], f = a.slot[n * 3 + 2];
        if (c >= 0) {
            row = ((int64_t)c * a.T + t) * a.F + f;
            img = (int64_t)f - a.f0;
        }
    } else {
        row = n;
        img = a.image_idx ? (int64_t)a.image_idx[n] : 0;
    }
    float r[4] = {0.f, 0.f, 0.f, 0.f};
    bool ok = row >= 0 && img >= 0 && img < a.Fi;
    if (row >= 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double b = a.boxes_f64 ? static_cast<const double *>(a.boxes)[row * a.ld + q]
                                         : (double)static_cast<const float *>(a.boxes)[row * a.ld + q];
            r[q] = (float)(b * a.box_scale);
            const float m = r[q] * a.spatial_scale;
            ok = ok && (r[q] - r[q] == 0.f) && fabsf(m) <= 16777216.0f;
        }
    }
    const int ph = a.ph, pw = a.pw;
    if (ok) {
        if constexpr (ALIGN) {
            const float off = a.aligned ? 0.5f : 0.f;
            const int ny = ph * a.sampling, nx = pw * a.sampling;
            for (int j = threadIdx.x; j < ny + nx; j += 256) {
                const int ax = j >= ny ? 1 : 0;                       // 0: rows (y1, y2), 1: columns (x1, x2)
                const float s = r[1 - ax] * a.spatial_scale - off;
                float ext = r[3 - ax] * a.spatial_scale - off - s;
                if (!a.aligned && ext < 1.0f) ext = 1.0f;
                const float b = ext / (float)(ax ? pw : ph);
                const int e = ax ? j - ny : j;
                roi_align_sample(e, a.sampling, s, b, ax ? a.Wf : a.Hf, s_lo[ax][e], s_hi[ax][e], s_l[ax][e], s_h[ax][e]);
            }
        } else {
            for (int j = threadIdx.x; j < ph + pw; j += 256) {
                const int ax = j >= ph ? 1 : 0;
                const int c1 = (int)roundf(r[1 - ax] * a.spatial_scale), c2 = (int)roundf(r[3 - ax] * a.spatial_scale);
                int ext = c2 - c1 + 1;
                if (ext < 1) ext = 1;
                const int e = ax ? j - ph : j, size = ax ? a.Wf : a.Hf;
                const float b = (float)ext / (float)(ax ? pw : ph);
                int lo = (int)floorf((float)e * b) + c1, hi = (int)ceilf((float)(e + 1) * b) + c1;
                lo = lo < 0 ? 0 : lo > size ? size : lo;
                hi = hi < 0 ? 0 : hi > size ? size : hi;
                s_lo[ax][e] = lo;
                s_hi[ax][e] = hi;
            }
        }
    }
    __syncthreads();
    if (chunk == 0 && threadIdx.x == 0) a.ok[n] = ok ? 1 : 0;
    const int bins = ph * pw, Wf = a.Wf;
    const int64_t plane = (int64_t)a.Hf * Wf;
    const FeatT *src = static_cast<const FeatT *>(a.features) + (ok ? img : 0) * a.K * plane;
    FeatT *dst = static_cast<FeatT *>(a.pooled) + n * a.span;
    auto element = [&](int64_t k, int b) {
        const int p = b / pw, q = b - p * pw;
            float v = 0.f;
            if (ok) {
                const FeatT *f = src + k * plane;
                if constexpr (ALIGN) {
                    const int S = a.sampling;
                    float acc = 0.f;
                    for (int iy = 0; iy < S; ++iy) {
                        const int ylo = s_lo[0][p * S + iy], yhi = s_hi[0][p * S + iy];
                        const float ly = s_l[0][p * S + iy], hy = s_h[0][p * S + iy];
                        for (int ix = 0; ix < S; ++ix) {
                            const int xlo = s_lo[1][q * S + ix], xhi = s_hi[1][q * S + ix];
                            float val = 0.f;
                            if (ylo >= 0 && xlo >= 0) {
                                const float lx = s_l[1][q * S + ix], hx = s_h[1][q * S + ix];
                                const float w1 = hy * hx, w2 = hy * lx, w3 = ly * hx, w4 = ly * lx;
                                const float v1 = roi_widen<FeatT>(f[(int64_t)ylo * Wf + xlo]), v2 = roi_widen<FeatT>(f[(int64_t)ylo * Wf + xhi]);
                                const float v3 = roi_widen<FeatT>(f[(int64_t)yhi * Wf + xlo]), v4 = roi_widen<FeatT>(f[(int64_t)yhi * Wf + xhi]);
                                val = ((w1 * v1 + w2 * v2) + w3 * v3) + w4 * v4;
                            }
                            acc = acc + val;
                        }
                    }
                    v = acc / (float)(S * S);
                } else {
                    const int hs = s_lo[0][p], he = s_hi[0][p], ws = s_lo[1][q], we = s_hi[1][q];
                    if (he > hs && we > ws) {
                        v = -FLT_MAX;
                        for (int h = hs; h < he; ++h)
                            for (int w = ws; w < we; ++w) {
                                const float x = roi_widen<FeatT>(f[(int64_t)h * Wf + w]);
                                if (x > v) v = x;
                            }
                    }
                }
            }
            dst[k * bins + b] = patch_cast<FeatT>(v);
    };
    if constexpr (WPC) {          // a wave per channel, lanes over the bins
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const int64_t k1 = ((int64_t)chunk + 1) * kRoiWaveCh < a.K ? ((int64_t)chunk + 1) * kRoiWaveCh : a.K;
        for (int64_t k = (int64_t)chunk * kRoiWaveCh + wave; k < k1; k += 4)
            for (int b = lane; b < bins; b += 64) element(k, b);
    } else {                      // lanes over the span; (k, b) of e = k*bins + b advance with e += 256 without a division
        const int64_t e0 = (int64_t)chunk * kRoiChunk + threadIdx.x;
        const int64_t e1 = ((int64_t)chunk + 1) * kRoiChunk < a.span ? ((int64_t)chunk + 1) * kRoiChunk : a.span;
        int64_t k = e0 / bins;
        int b = (int)(e0 - k * bins);
        const int dk = 256 / bins, db = 256 - dk * bins;
        for (int64_t e = e0; e < e1; e += 256) {
            element(k, b);
            k += dk;
            b += db;
            if (b >= bins) {
                b -= bins;
                ++k;
            }
        }
    }
}

}  // namespace vdet
