// R-CNN windows on the device (vdet_rcnn_patches / vdet_tubelet_patches, include/vdet_hip.h): the step in front of the CNN
// scorers, rcnn_img_crop + im_transform (reference utils/common.py:208-280) for every box of a call in one launch, and
// sampling_boxes (vdet/tubelet_cls.py:136-142) with the caller's draw.  Everything up to the final cast is f64 and every
// product and sum a separate operation (the library is built with -ffp-contract=off): tests/patch_spec.py states the same
// arithmetic in numpy and the two are compared bit for bit.
//
// rcnn_patches_kernel<OutT, VEC>   one WAVE per (window, strip of kPatchRows patch rows), four per workgroup, on a 1-D grid
//     (the window count may exceed a 65 535 grid axis).  The wave index is made uniform with readfirstlane, so the box, the
//     slot row and the image index are scalar loads and the window geometry -- padding, Python-2 rounding, clipping, the crop
//     size and its place in the patch -- is computed once per wave, every lane holding the same registers.  A lane then owns
//     VEC consecutive elements of a row for the three channels: per element the source taps and f32 weights of OpenCV's
//     generic bilinear path, the 2x2 f64 blend, minus the mean, one cast.  A strip of one channel is one contiguous span of
//     the output and consecutive lanes hold consecutive VEC-groups, so every store instruction is a run of whole 16-byte
//     (f32, VEC = 4; 16-bit types, VEC = 8) pieces; VEC = 1 is the scalar form of sizes that are no multiple of 4.  The whole
//     patch is written, zeros outside the placed rectangle and for a window that is not ok.  Offsets into the output are
//     64-bit.  The source pixels are read through the vector cache: a frame is a few MB and stays in L2.
// tubelet_slots_kernel   one workgroup of 1024.  Per chunk of 1024 slots in the order ((f-f0)*C + c)*T + t: a ballot of
//     "present" per wave, the sixteen wave counts through LDS, a popcount prefix inside the wave -> the ordinal of every
//     present slot.  Writes (c,t,f) at the ordinal while it is below cap, -1 rows behind the count, the TRUE count, and
//     latches kStPatchCap when it exceeds cap.  No atomics on a result path.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vdet {

constexpr int kStPatchCap = 1024;     // vdet_tubelet_patches: more present slots in the frame range than cap
constexpr int kPatchRows = 16;        // patch rows per wave
constexpr int kPatchMaxS = 1024;
constexpr int kPatchMaxHW = 32767;
constexpr int kPatchMaxNum = 255;

struct PatchBf16 { uint16_t u; };

struct PatchArgs {
    const uint8_t *images;      // [Fi,H,W,3]
    int Fi, H, W;
    const void *boxes;          // rows of ld elements, f32 or f64; columns 0..3 are x1,y1,x2,y2 (1-based, inclusive)
    int boxes_f64, ld;
    const int32_t *image_idx;   // [N] or null (image 0)           -- array form
    const double *offsets;      // [N,num,4] or null
    int num;
    const int32_t *slot;        // [M,3] (c,t,f) or null           -- tubelet form: box = row ((c*T + t)*F + f), image f - f0
    int T;
    int64_t F, f0;
    const double *mean;         // [3] or null
    int S, padding, square, nstrips;
    int64_t M;                  // windows
    void *patches;              // [M,3,S,S] OutT
    uint8_t *ok;                // [M]
    double *sboxes;             // [M,4] or null
};

struct PatchGeom {
    int ok;
    int x1, y1, sw, sh;         // source rectangle: origin and size
    int cw, ch, pw, ph;         // resized size and its place in the patch
};

__host__ __device__ __forceinline__ bool patch_finite(double x) { return x - x == 0.0; }

// rcnn_img_crop's geometry (:209-252).  max / min are Python's: max(0, x) is x only when x > 0.
__host__ __device__ inline PatchGeom patch_geometry(const double in[4], int H, int W, int S, int padding, int square)
{
    PatchGeom g = {0, 0, 0, 0, 0, S, S, 0, 0};
    if (!(patch_finite(in[0]) && patch_finite(in[1]) && patch_finite(in[2]) && patch_finite(in[3]))) return g;
    double x1 = in[0] - 1.0, y1 = in[1] - 1.0, x2 = in[2] - 1.0, y2 = in[3] - 1.0;
    if (padding > 0 || square) {
        const double scale = (double)S * 1.0 / (double)(S - padding * 2);
        double hh = (y2 - y1 + 1.0) / 2.0;
        double hw = (x2 - x1 + 1.0) / 2.0;
        const double cx = x1 + hw, cy = y1 + hh;
        if (square) {
            if (hh > hw) hw = hh; else hh = hw;
        }
        x1 = round(cx - hw * scale);       // C round(): half away from zero, Python 2's
        y1 = round(cy - hh * scale);
        x2 = round(cx + hw * scale);
        y2 = round(cy + hh * scale);
        if (!(patch_finite(x1) && patch_finite(y1) && patch_finite(x2) && patch_finite(y2))) return g;
        const double uh = y2 - y1 + 1.0, uw = x2 - x1 + 1.0;
        const double px = (-x1 > 0.0) ? -x1 : 0.0;
        const double py = (-y1 > 0.0) ? -y1 : 0.0;
        x1 = (x1 > 0.0) ? x1 : 0.0;
        y1 = (y1 > 0.0) ? y1 : 0.0;
        x2 = (x2 < (double)(W - 1)) ? x2 : (double)(W - 1);
        y2 = (y2 < (double)(H - 1)) ? y2 : (double)(H - 1);
        const double chh = y2 - y1 + 1.0, cww = x2 - x1 + 1.0;
        if (!(uh >= 1.0 && uw >= 1.0 && chh >= 1.0 && cww >= 1.0)) return g;
        // from here 0 <= x1 <= x2 <= W-1 (and y), px <= uw, py <= uh: every product below is at most S * max(H, W)
        const double sx = (double)S * 1.0 / uw, sy = (double)S * 1.0 / uh;
        g.cw = (int)round(cww * sx);
        g.ch = (int)round(chh * sy);
        g.pw = (int)round(px * sx);
        g.ph = (int)round(py * sy);
        if (g.ph + g.ch > S) g.ch = S - g.ph;
        if (g.pw + g.cw > S) g.cw = S - g.pw;
        if (g.cw < 1 || g.ch < 1) return g;
    } else {
        x1 = trunc(x1); y1 = trunc(y1); x2 = trunc(x2); y2 = trunc(y2);
        if (!(0.0 <= x1 && x1 <= x2 && x2 <= (double)(W - 1) && 0.0 <= y1 && y1 <= y2 && y2 <= (double)(H - 1))) return g;
    }
    g.x1 = (int)x1;
    g.y1 = (int)y1;
    g.sw = (int)x2 - g.x1 + 1;
    g.sh = (int)y2 - g.y1 + 1;
    g.ok = 1;
    return g;
}

// one axis of the bilinear resize: destination index d of dst, source extent src -> taps s0, s1 and their f64 weights
__host__ __device__ __forceinline__ void patch_axis(int d, int src, int dst, int &s0, int &s1, double &w0, double &w1)
{
    float f = (float)(((double)d + 0.5) * ((double)src / (double)dst) - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) { s = 0; f = 0.f; }
    if (s >= src - 1) { s = src - 1; f = 0.f; }
    s0 = s;
    s1 = (s + 1 < src) ? s + 1 : src - 1;
    w0 = (double)(1.f - f);
    w1 = (double)f;
}

// channel k of patch element (y, x) of a window that is ok, with (y, x) inside the placed rectangle
__host__ __device__ __forceinline__ double patch_blend(const uint8_t *img, int W, int k, int x0, int x1, double a0, double a1, int y0,
                                                       int y1, double b0, double b1)
{
    const uint8_t *r0p = img + (int64_t)y0 * W * 3 + k, *r1p = img + (int64_t)y1 * W * 3 + k;
    const double r0 = (double)r0p[x0 * 3] * a0 + (double)r0p[x1 * 3] * a1;
    const double r1 = (double)r1p[x0 * 3] * a0 + (double)r1p[x1 * 3] * a1;
    return r0 * b0 + r1 * b1;
}

template <typename OutT> __device__ __forceinline__ OutT patch_cast(float v);
template <> __device__ __forceinline__ float patch_cast<float>(float v) { return v; }
template <> __device__ __forceinline__ _Float16 patch_cast<_Float16>(float v) { return (_Float16)v; }     // round to nearest even
template <> __device__ __forceinline__ PatchBf16 patch_cast<PatchBf16>(float v)
{
    uint32_t u = __float_as_uint(v);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return PatchBf16{(uint16_t)((u >> 16) | 0x40u)};     // NaN stays NaN
    u += 0x7FFFu + ((u >> 16) & 1u);                                                         // round to nearest even
    return PatchBf16{(uint16_t)(u >> 16)};
}

template <typename OutT, int VEC> struct alignas(sizeof(OutT) * VEC) PatchPack { OutT e[VEC]; };

template <typename OutT, int VEC>
__global__ __launch_bounds__(256) void rcnn_patches_kernel(const PatchArgs a)
{
    const int lane = threadIdx.x & 63;
    const int64_t wv = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (wv >= a.M * a.nstrips) return;
    const int64_t m = wv / a.nstrips;
    const int strip = (int)(wv - m * a.nstrips);
    const int S = a.S;
    // the window's box and image: the same for every lane
    int64_t row = -1;
    int64_t img = 0;
    int j = 0;
    if (a.slot) {
        const int c = a.slot[m * 3], t = a.slot[m * 3 + 1], f = a.slot[m * 3 + 2];
        if (c >= 0) {
            row = ((int64_t)c * a.T + t) * a.F + f;
            img = (int64_t)f - a.f0;
        }
    } else {
        row = m / (a.num + 1);
        j = (int)(m - row * (a.num + 1));
        img = a.image_idx ? (int64_t)a.image_idx[row] : 0;
    }
    double b[4] = {0.0, 0.0, 0.0, 0.0};
    if (row >= 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            b[q] = a.boxes_f64 ? static_cast<const double *>(a.boxes)[row * a.ld + q]
                               : (double)static_cast<const float *>(a.boxes)[row * a.ld + q];
        if (j > 0) {       // sampling_boxes: box + offsets * [w,h,w,h], w = x2-x1, h = y2-y1
            const double *o = a.offsets + (row * a.num + (j - 1)) * 4;
            const double w = b[2] - b[0], h = b[3] - b[1];
            b[0] = b[0] + o[0] * w;
            b[1] = b[1] + o[1] * h;
            b[2] = b[2] + o[2] * w;
            b[3] = b[3] + o[3] * h;
        }
    }
    PatchGeom g = patch_geometry(b, a.H, a.W, S, a.padding, a.square);
    const bool ok = row >= 0 && img >= 0 && img < a.Fi && g.ok;
    if (strip == 0) {
        if (lane == 0) a.ok[m] = ok ? 1 : 0;
        if (a.sboxes && lane < 4) a.sboxes[m * 4 + lane] = lane == 0 ? b[0] : lane == 1 ? b[1] : lane == 2 ? b[2] : b[3];
    }
    const uint8_t *src = a.images + (ok ? img : 0) * a.H * a.W * 3 + ((int64_t)g.y1 * a.W + g.x1) * 3;
    double mean[3] = {0.0, 0.0, 0.0};
    if (a.mean) { mean[0] = a.mean[0]; mean[1] = a.mean[1]; mean[2] = a.mean[2]; }
    const int r0 = strip * kPatchRows;
    const int r1 = (r0 + kPatchRows < S) ? r0 + kPatchRows : S;
    const int gpr = S / VEC;
    const int ngroups = (r1 - r0) * gpr;
    OutT *base = static_cast<OutT *>(a.patches) + m * 3 * S * S;
    for (int q = lane; q < ngroups; q += 64) {
        const int yq = q / gpr;
        const int y = r0 + yq, x = (q - yq * gpr) * VEC;
        PatchPack<OutT, VEC> out[3];
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int i = 0; i < VEC; ++i) out[k].e[i] = patch_cast<OutT>(0.f);
        const int dy = y - g.ph;
        if (ok && dy >= 0 && dy < g.ch && x + VEC > g.pw && x < g.pw + g.cw) {
            int y0, y1;
            double b0, b1;
            patch_axis(dy, g.sh, g.ch, y0, y1, b0, b1);
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                const int dx = x + i - g.pw;
                if (dx < 0 || dx >= g.cw) continue;
                int x0, x1;
                double a0, a1;
                patch_axis(dx, g.sw, g.cw, x0, x1, a0, a1);
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double v = patch_blend(src, a.W, k, x0, x1, a0, a1, y0, y1, b0, b1);
                    out[k].e[i] = patch_cast<OutT>(a.mean ? (float)(v - mean[k]) : (float)v);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k)
            *reinterpret_cast<PatchPack<OutT, VEC> *>(base + ((int64_t)k * S + y) * S + x) = out[k];
    }
}

// slot compaction of the tubelet form: see the head of this file.  tracks rows of ld elements, [C,T,F,ld]
__global__ __launch_bounds__(1024) void tubelet_slots_kernel(const void *tracks, int tracks_f64, int ld, const int32_t *ntracks, int C,
                                                             int T, int64_t F, int64_t f0, int64_t f1, int64_t cap, int32_t *slot,
                                                             int32_t *count, int *status)
{
    __shared__ int wsum[16];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t L = (f1 - f0) * C * T;
    int64_t n = 0;
    for (int64_t i0 = 0; i0 < L; i0 += 1024) {
        const int64_t i = i0 + threadIdx.x;
        bool present = false;
        int c = 0, t = 0;
        int64_t f = 0;
        if (i < L) {
            const int64_t fc = i / T;
            t = (int)(i - fc * T);
            f = f0 + fc / C;
            c = (int)(fc % C);
            if (t < ntracks[c]) {
                const int64_t e = (((int64_t)c * T + t) * F + f) * ld;
                if (tracks_f64) {
                    const double x = static_cast<const double *>(tracks)[e];
                    present = x == x;
                } else {
                    const float x = static_cast<const float *>(tracks)[e];
                    present = x == x;
                }
            }
        }
        const unsigned long long mk = __ballot(present);
        if (lane == 0) wsum[w] = __popcll(mk);
        __syncthreads();
        int before = 0, total = 0;
        for (int k = 0; k < 16; ++k) {
            const int s = wsum[k];
            if (k < w) before += s;
            total += s;
        }
        if (present) {
            const int64_t o = n + before + __popcll(mk & ((1ull << lane) - 1ull));
            if (o < cap) {
                slot[o * 3] = c;
                slot[o * 3 + 1] = t;
                slot[o * 3 + 2] = (int32_t)f;
            }
        }
        n += total;
        __syncthreads();
    }
    for (int64_t o = n + threadIdx.x; o < cap; o += 1024) {
        slot[o * 3] = -1;
        slot[o * 3 + 1] = -1;
        slot[o * 3 + 2] = -1;
    }
    if (threadIdx.x == 0) {
        *count = (int32_t)n;
        if (n > cap) atomicOr(status, kStPatchCap);
    }
}

}  // namespace vdet
