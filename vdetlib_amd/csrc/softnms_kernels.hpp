// Soft-NMS (Bodla et al., ICCV 2017) of the per-frame detection lists of tracknms_kernels.hpp: instead of deleting a row that
// overlaps a better one, its score is decayed -- 'linear' s *= 1 - ovr where ovr >= thresh, 'gauss' s *= exp(-ovr^2 / sigma)
// for every pair -- and the list is emitted in the order of the CURRENT scores.  Semantics in full: include/vdet_hip.h
// (vdet_soft_nms_tracks); the rule in numpy float32: tests/softnms_spec.py, which the kernel equals on bits.
//
// The LIST and the launch shape are tracknms_kernels.hpp's, through its shared pieces tn_load_row, tn_store_row / tn_store_pad
// and tn_close.  The round below is this rule's own loop, not tn_select.  The prologue is still written out here and is
// tn_open + TnLds statement for statement: with the two calls the round loop is the same instructions, but its head moves off
// the 64-byte line it starts on (0x..340 -> 0x..39c in the code object) and every leg of devtools/bench_softnms.py measured
// 1.0 - 2.0 % slower on the MI355X; with the prologue here the kernel's code up to the loop is the old one.
//
// Per wave, LDS: box [n] float4, COMPOSITE [n] 64-bit, current score [n] f32, area [n] f32, n = top_still + T of THE CALL
// (32 bytes per candidate: 4 waves up to 511 candidates, 2 up to 1023, 1 at the limit of 1024).
//   composite = score_key(s) << 32 | j  while the row is alive,  = rank + 1 once it is emitted,  = 0 absent or removed.
// score_key folds -0.0 into +0.0 and cannot give the score back, so the f32 score stands beside it: the home that keeps its
// bits, and -- a row's score never changes after it is emitted -- the final score the output sweep writes.
// Entry j is read and written by lane j & 63 alone; only the boxes and areas are read across lanes (written once, one fence).
// A ROUND: the wave maximum of the alive composites is the next emitted row (descending current score, -0.0 == +0.0, equal
// scores by descending index); every other alive row is an evaluated pair against it -- ovr in the reference's operation
// order with the correctly rounded f32 division, a zero union latches kStDivZero, a NaN ovr changes nothing -- its score is
// decayed, its composite rebuilt or cleared (NaN or below the floor), and the same sweep carries the next maximum.
// Cost: emitted x ceil(n / 64) divisions per lane and six 64-bit shuffles per emitted row; rounds = rows emitted, not the
// survivors of a hard NMS.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tracknms_kernels.hpp"  // TrackNmsArgs, TnList, TnRow, the shared pieces, tn_wave_max, kTnMaxList

namespace vdet {

constexpr int kSnBytesPerCand = 32;  // float4 box + 64-bit composite + f32 score + f32 area
constexpr int kSnLinear = 0, kSnGauss = 1;
constexpr double kSnSigmaMin = 1.0 / 64;   // with ovr <= 1 the Gaussian weight's argument -ovr^2 / sigma stays in [-64, 0]

struct SoftNmsArgs {
    TrackNmsArgs tn;            // the list sources and the outputs of vdet_nms_tracks; tn.oscore = the decayed score widened
    double *oscore0;            // [C,R,F] the source's own unrounded score
    int method;
    float sigma32, min32;       // (float)sigma, (float)min_score
};

// The Gaussian weight's exponential for x <= 0: tests/softnms_spec.py g, operation by operation (the TU is built with
// -ffp-contract=off: every multiply and add below is one correctly rounded f32 operation).  Below the cut +0.0; everywhere
// else the result is a normal float, so ldexp is exact.  Why the argument goes to a grid first: the spec's docstring.
__device__ __forceinline__ float sn_exp(float x)
{
    if (x < -87.0f) return 0.0f;
    x = __builtin_rintf(x * 1048576.0f) * 9.5367431640625e-7f;      // to a multiple of 2^-20 (exact): what makes the weight monotone
    const float kf = __builtin_rintf(x * 1.4426950408889634f);
    float r = x - kf * 0.693359375f;
    r = r - kf * -2.12194440e-4f;
    float p = 0.0013814590638503432f;
    p = p * r + 0.0083687175065279f;
    p = p * r + 0.04166838899254799f;
    p = p * r + 0.1666652113199234f;
    p = p * r + 0.4999999403953552f;
    p = p * r + 1.0f;
    p = p * r + 1.0f;
    return ldexpf(p, (int)kf);
}

// utils/nms.pyx:57-64, box i = the emitted row.  zero: the union is 0 (the reference's ZeroDivisionError)
__device__ __forceinline__ float sn_overlap(float4 bi, float iarea, float4 bj, float jarea, bool &zero)
{
    const float xx1 = ref_max(bi.x, bj.x);
    const float yy1 = ref_max(bi.y, bj.y);
    const float xx2 = ref_min(bi.z, bj.z);
    const float yy2 = ref_min(bi.w, bj.w);
    const float w = ref_max(0.0f, (xx2 - xx1) + 1.0f);
    const float h = ref_max(0.0f, (yy2 - yy1) + 1.0f);
    const float inter = w * h;
    const float uni = (iarea + jarea) - inter;
    if (uni == 0.0f) zero = true;
    return inter / uni;
}

__global__ __launch_bounds__(256) void softnms_kernel(const SoftNmsArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char sn_smem[];
    const TrackNmsArgs &g = a.tn;
    const int lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    TnList m;
    const int v = blockIdx.y;
    int64_t f0 = 0;
    m.F = g.F;
    if (g.vids) { const VidDesc vd = g.vids[v]; f0 = vd.f0; m.F = vd.F; }
    const int64_t s = (int64_t)blockIdx.x * nw + w;
    if (s >= (int64_t)g.C * m.F) return;
    m.c = (int)(s / m.F);
    m.f = (int)(s - (int64_t)m.c * m.F);
    m.fg = f0 + m.f;
    m.tbase = (int64_t)g.C * g.T * f0 + (int64_t)m.c * g.T * m.F + m.f;
    m.obase = (int64_t)g.C * g.R * f0 + (int64_t)m.c * g.R * m.F + m.f;
    // [nw][nmax] of each: boxes (16 B), composites (8 B), scores (4 B), areas (4 B)
    const size_t all = (size_t)nw * g.nmax, mine = (size_t)w * g.nmax;
    float4 *sbox = reinterpret_cast<float4 *>(sn_smem) + mine;
    unsigned long long *scomp = reinterpret_cast<unsigned long long *>(sn_smem + all * 16) + mine;
    float *sscore = reinterpret_cast<float *>(sn_smem + all * 24) + mine;
    float *sarea = reinterpret_cast<float *>(sn_smem + all * 28) + mine;

    bool badkeep = false;
    m.ns = 0;
    if (g.top_still > 0) {
        const int kc = g.keep_cnt[m.fg * g.C + m.c];
        if (kc < 0 || kc > g.cap) badkeep = true;
        else m.ns = kc < g.top_still ? kc : g.top_still;
    }
    int nt = 0;
    if (g.T > 0) {
        nt = g.ntracks[(int64_t)v * g.C + m.c];
        nt = nt < 0 ? 0 : (nt > g.T ? g.T : nt);
    }
    m.n = m.ns + nt;                                     // (<= top_still + T = nmax)

    // gather: a row below the floor is removed before the first round
    unsigned long long best = 0ull;
    for (int j = lane; j < m.n; j += 64) {
        TnRow r;
        unsigned long long k = 0ull;
        if (tn_load_row(g, m, j, r, badkeep) && !(r.s32 < a.min32)) {
            sbox[j] = r.box;
            sarea[j] = box_area(r.box);
            sscore[j] = r.s32;
            k = ((unsigned long long)score_key(r.s32) << 32) | (unsigned)j;
        }
        scomp[j] = k;
        best = k > best ? k : best;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();

    // rounds
    int emitted = 0;
    bool zero = false;
    const bool gauss = a.method == kSnGauss;
    for (;;) {
        const unsigned long long top = tn_wave_max(best);
        const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(top >> 32));
        if (hi == 0u) break;
        const int i = __builtin_amdgcn_readfirstlane((int)(unsigned)top);
        const float4 bi = sbox[i];
        const float ai = sarea[i];
        best = 0ull;
        for (int j = lane; j < m.n; j += 64) {
            unsigned long long k = scomp[j];
            if ((k >> 32) == 0ull) continue;
            if (j == i) { scomp[j] = (unsigned long long)(emitted + 1); continue; }
            const float ovr = sn_overlap(bi, ai, sbox[j], sarea[j], zero);
            float sj = sscore[j];
            bool changed = false;
            if (gauss) {
                if (ovr == ovr) { sj = sj * sn_exp(-(ovr * ovr) / a.sigma32); changed = true; }
            } else if (ovr >= g.t32) {
                sj = sj * (1.0f - ovr);
                changed = true;
            }
            if (changed) {
                if (sj != sj || sj < a.min32) k = 0ull;
                else { sscore[j] = sj; k = ((unsigned long long)score_key(sj) << 32) | (unsigned)j; }
                scomp[j] = k;
            }
            best = k > best ? k : best;
        }
        ++emitted;
    }

    // output: the emitted rows at their ranks with their final scores, the fill behind the count
    for (int j = lane; j < m.n; j += 64) {
        const unsigned long long k = scomp[j];
        if ((k >> 32) != 0ull || k == 0ull) continue;
        const int r = (int)k - 1;
        if (r >= g.R) continue;
        TnRow row;
        bool dummy = false;
        tn_load_row(g, m, j, row, dummy);
        const float sj = sscore[j];
        const int64_t e = m.obase + (int64_t)r * m.F;
        tn_store_row(g, e, row.box, sj, (double)sj, row.src);
        a.oscore0[e] = row.s64;
    }
    for (int r = (emitted < g.R ? emitted : g.R) + lane; r < g.R; r += 64) {
        const int64_t e = m.obase + (int64_t)r * m.F;
        tn_store_pad(g, e);
        a.oscore0[e] = __longlong_as_double(0x7FF8000000000000ll);
    }
    tn_close(g, m, lane, emitted, badkeep, zero);
}

}  // namespace vdet

