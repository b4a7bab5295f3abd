// Seq-NMS (Han et al. 2016) on per-frame detections in the tubelet layout: link the boxes of neighbouring frames that overlap,
// take the sequence with the largest score sum by dynamic programming, give its boxes the sequence's average (or maximum)
// score, suppress what they overlap in their own frames, repeat.  The reference library has no function for it; the rule is
// tests/seqnms_spec.py, which the device matches on bits.  Semantics in full: include/vdet_hip.h (vdet_seq_nms).
//
// A NODE is row (r, f) of tracks [C,R,F,5] with r < ntracks[c], x1 not NaN and a finite score (f64).  hit(a, b, t) is the f32
// arithmetic of pair_pred (nms_kernels.hpp) with the QUOTIENT rule: uni > 0 and (double)(inter / uni) >= t -- one f32
// division, no divide-free form, so there is no knife edge to fall off.
//
// TWO kernels, no block ever waits for another, every loop bound is a number the host knows (R, W, F_v, max_seqs, rounds):
//
// seqnms_link_kernel   grid (C * Fmax, V), one block per (class, frame), one thread per row.  Owns and writes EVERY output slot
//   of its frame (nodes: box bits, (float)score, score, seq = -1; the rest NaN / INT32_MIN), so whatever the rounds do not
//   reach is already final; the block of frame 0 poisons the class's sequence table.  Scratch: the live bits [C,Ftot,W] u32
//   (W = ceil(R / 32); a wave ballot per word) and the LINK bits [C,Ftot,R,W] u32 -- word w of row (r, f) holds
//   hit(box[32w+j, f-1], box[r, f], link_thres) in bit j, the previous frame's boxes in LDS, R*R quotients per block.  The
//   bits do not depend on which nodes are live: the rounds never compute an IoU between frames again.
//
// seqnms_rounds_kernel grid (C, V), one block per (video, class), thread r = row r, `rounds` rounds per launch; the host
//   enqueues ceil((max_seqs + 1) / rounds) launches with no wait between them (rounds * Fmax <= kSqFrameSteps bounds a
//   launch).  What carries over is in global memory: the live bits, nseq, and a done flag per (video, class).  One round:
//     forward   frames ascending, ONE barrier per frame: thread r reads its live bit, its f64 score (the score output, which
//               holds a live node's own score) and its W link words -- all three fetched one frame ahead -- and walks the set
//               bits of link & live(f-1) over the previous frame's best[] in LDS (double-buffered; -1 for rows that are not
//               live): best = s + max, ptr = the lowest q attaining it, and the running maximum of s along the path.  ptr is an
//               int16 per node in LDS, [F_v, Rp]; when (F_v * Rp + F_v) * 2 bytes exceed kSqLdsBudget it lies in global
//               scratch instead (VDET_SEQNMS_LDS=0 forces that; vdet_query 14 tells).  Same results.
//     end node  every thread keeps its own best (strict >, so its lowest frame), one block reduction: value, then lowest
//               frame, then lowest slot.
//     path      thread 0 follows ptr back (<= F_v dependent LDS reads), writes path[f], the sum, length and end of the sequence.
//     suppress  frames of the path, no barrier: thread r tests its row against the path node of the frame if it is live;
//               members get (float)new / new / k, suppressed rows NaN / -2; the live word of 32 rows is rewritten by the
//               lane that owns it from a ballot -- no atomics.
//   The terminal iteration (k == max_seqs) scans the live words for `exhausted`.
// All results leave through plain vector stores.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nms_kernels.hpp"       // box_area, ref_max, ref_min
#include "batch_kernels.hpp"     // VidDesc

namespace vdet {

constexpr int kSqMaxR = 256;                 // rows per (frame, class): one thread each
constexpr int kSqMaxSeqs = 4096;
constexpr int kSqMaxW = kSqMaxR / 32;
constexpr int kSqLdsBudget = 128 * 1024;     // bytes of ptr + path in LDS (gfx950: 160 KiB per workgroup, 9 KiB are static)
constexpr int kSqFrameSteps = 16384;         // frames a block passes per launch: rounds per launch = max(1, this / Fmax)
constexpr int kSqSeqNone = INT32_MIN, kSqSeqLeft = -1, kSqSeqSupp = -2;

struct SeqNmsArgs {
    const float *tracks;        // [C,R,F,5]  (batch: video v at element C*R*f0)
    const int32_t *ntracks;     // [V,C]
    const void *score;          // [C,R,F] f32 / f64, or null: column 4
    const VidDesc *vids;        // null: one video of F frames
    int F, Ftot, C, R, W, Rp, S, score_f64, rescore, rounds, ptr_lds;
    double link_t, nms_t, min_score;
    float *otracks;             // [C,R,F,5]
    double *oscore;             // [C,R,F]
    int32_t *oseq;              // [C,R,F]
    int32_t *ontracks, *onseq;  // [V,C]
    double *oseq_sum;           // [V,C,S]
    int32_t *oseq_len;          // [V,C,S]
    int32_t *oseq_end;          // [V,C,S,2]
    uint8_t *oexh;              // [V,C]
    uint32_t *link;             // [C,Ftot,R,W]
    uint32_t *live;             // [C,Ftot,W]
    int32_t *done;              // [V,C]
    int16_t *gptr;              // [C,Ftot,Rp+1] when !ptr_lds: video v at C*(Rp+1)*f0, then per class F_v*Rp ptr and F_v path
};

__device__ __forceinline__ bool sq_hit(float4 a, float4 b, double t)
{
    const float aa = box_area(a), ab = box_area(b);
    const float xx1 = ref_max(a.x, b.x);
    const float yy1 = ref_max(a.y, b.y);
    const float xx2 = ref_min(a.z, b.z);
    const float yy2 = ref_min(a.w, b.w);
    const float w = ref_max(0.0f, (xx2 - xx1) + 1.0f);
    const float h = ref_max(0.0f, (yy2 - yy1) + 1.0f);
    const float inter = w * h;
    const float uni = (aa + ab) - inter;
    return uni > 0.0f && (double)(inter / uni) >= t;
}

__device__ __forceinline__ float4 sq_box(const float *row) { return make_float4(row[0], row[1], row[2], row[3]); }

__global__ __launch_bounds__(256) void seqnms_link_kernel(const SeqNmsArgs g)
{
    __shared__ float4 sprev[kSqMaxR];
    const int v = blockIdx.y;
    const int Fmax = g.F;
    int f0 = 0, Fv = g.F;
    if (g.vids) { const VidDesc vd = g.vids[v]; f0 = vd.f0; Fv = vd.F; }
    const int c = (int)(blockIdx.x / (unsigned)Fmax), f = (int)(blockIdx.x % (unsigned)Fmax);
    if (f >= Fv) return;                                  // (the whole block)
    const int r = threadIdx.x, lane = r & 63, wv = r >> 6;
    const int64_t vc = (int64_t)v * g.C + c;
    int nt = g.ntracks[vc];
    nt = nt < 0 ? 0 : (nt > g.R ? g.R : nt);
    const float qnan = __uint_as_float(0x7FC00000u);
    bool node = false;
    float4 box = make_float4(qnan, qnan, qnan, qnan);
    if (r < g.R) {
        const int64_t e = (int64_t)g.C * g.R * f0 + ((int64_t)c * g.R + r) * Fv + f;
        const float *row = g.tracks + e * 5;
        box = sq_box(row);
        double s;
        if (!g.score) s = (double)row[4];
        else if (g.score_f64) s = static_cast<const double *>(g.score)[e];
        else s = (double)static_cast<const float *>(g.score)[e];
        node = r < nt && box.x == box.x && s - s == 0.0;          // (finite: neither NaN nor +-inf)
        float *o = g.otracks + e * 5;
        if (node) {
            o[0] = box.x; o[1] = box.y; o[2] = box.z; o[3] = box.w; o[4] = (float)s;
            g.oscore[e] = s;
            g.oseq[e] = kSqSeqLeft;
        } else {
            o[0] = qnan; o[1] = qnan; o[2] = qnan; o[3] = qnan; o[4] = qnan;
            g.oscore[e] = __longlong_as_double(0x7FF8000000000000ll);
            g.oseq[e] = kSqSeqNone;
        }
        if (f > 0) sprev[r] = sq_box(row - 5);
    }
    const unsigned long long bal = __ballot(node);
    const int64_t lw = ((int64_t)c * g.Ftot + f0 + f) * g.W;
    if (lane == 0 && 2 * wv < g.W) g.live[lw + 2 * wv] = (uint32_t)bal;
    if (lane == 32 && 2 * wv + 1 < g.W) g.live[lw + 2 * wv + 1] = (uint32_t)(bal >> 32);
    __syncthreads();
    if (r < g.R) {
        uint32_t *out = g.link + (((int64_t)c * g.Ftot + f0 + f) * g.R + r) * g.W;
        for (int w = 0; w < g.W; ++w) {
            uint32_t word = 0u;
            if (f > 0) {
                for (int j = 0; j < 32; ++j) {
                    const int q = 32 * w + j;
                    if (q < g.R && sq_hit(sprev[q], box, g.link_t)) word |= 1u << j;
                }
            }
            out[w] = word;
        }
    }
    if (f == 0) {
        for (int k = r; k < g.S; k += (int)blockDim.x) {
            const int64_t i = vc * g.S + k;
            g.oseq_sum[i] = __longlong_as_double(0x7FF8000000000000ll);
            g.oseq_len[i] = 0;
            g.oseq_end[2 * i] = -1;
            g.oseq_end[2 * i + 1] = -1;
        }
        if (r == 0) { g.ontracks[vc] = nt; g.onseq[vc] = 0; g.oexh[vc] = 0; g.done[vc] = 0; }
    }
}

struct SqCand { double v, m; int f, r; };      // r < 0: none

__device__ __forceinline__ bool sq_better(const SqCand &a, const SqCand &b)
{
    if (a.r < 0) return false;
    if (b.r < 0) return true;
    if (a.v != b.v) return a.v > b.v;
    if (a.f != b.f) return a.f < b.f;
    return a.r < b.r;
}

__global__ __launch_bounds__(256) void seqnms_rounds_kernel(const SeqNmsArgs g)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char sq_smem[];
    __shared__ double sbest[2][kSqMaxR], smx[2][kSqMaxR];
    __shared__ uint32_t slive[2][kSqMaxW];
    __shared__ SqCand scand[4];
    __shared__ int sctl[3];                    // first frame, last frame, go
    __shared__ double snew;
    const int c = blockIdx.x, v = blockIdx.y;
    const int64_t vc = (int64_t)v * g.C + c;
    if (g.done[vc] != 0) return;               // (the whole block; nothing below writes it before the block's last barrier)
    int f0 = 0, Fv = g.F;
    if (g.vids) { const VidDesc vd = g.vids[v]; f0 = vd.f0; Fv = vd.F; }
    const int r = threadIdx.x, lane = r & 63, wv = r >> 6, nw = (int)blockDim.x >> 6;
    const int R = g.R, W = g.W, Rp = g.Rp;
    const bool active = r < R;
    int16_t *ptrs = g.ptr_lds ? reinterpret_cast<int16_t *>(sq_smem) : g.gptr + ((int64_t)g.C * f0 + (int64_t)c * Fv) * (Rp + 1);
    int16_t *path = ptrs + (int64_t)Fv * Rp;
    const int64_t e0 = (int64_t)g.C * R * f0 + ((int64_t)c * R + (active ? r : 0)) * Fv;   // element of (r, frame 0)
    const int64_t fg0 = (int64_t)c * g.Ftot + f0;                                          // (class, frame 0) of the scratch
    uint32_t *lv = g.live + fg0 * W;                                                       // [F_v, W]
    const uint32_t *lk = g.link + (fg0 * R + (active ? r : 0)) * W;                        // + f * R * W
    const int myw = (active ? r : 0) >> 5, myb = r & 31;
    const double qnan64 = __longlong_as_double(0x7FF8000000000000ll);
    const float qnan = __uint_as_float(0x7FC00000u);
    int k = g.onseq[vc];

    for (int it = 0; it < g.rounds; ++it) {
        if (k >= g.S) {                        // the terminal iteration: is anything left?
            int any = 0;
            for (int i = r; i < Fv * W; i += (int)blockDim.x) any |= lv[i] != 0u;
            any = __syncthreads_or(any);
            if (r == 0) { g.oexh[vc] = any ? 0 : 1; g.done[vc] = 1; }
            return;
        }
        // ---- forward pass
        SqCand mine{0.0, 0.0, 0, -1};
        uint32_t nl = 0u, nlw[kSqMaxW];
        double ns = 0.0;
#pragma unroll
        for (int w = 0; w < kSqMaxW; ++w) nlw[w] = 0u;
        if (active) { nl = (lv[myw] >> myb) & 1u; ns = g.oscore[e0]; }
        for (int f = 0; f < Fv; ++f) {
            const uint32_t cl = nl;
            const double cs = ns;
            uint32_t clw[kSqMaxW];
#pragma unroll
            for (int w = 0; w < kSqMaxW; ++w) clw[w] = nlw[w];
            if (active && f + 1 < Fv) {        // the next frame's operands, in flight across the barrier
                nl = (lv[(int64_t)(f + 1) * W + myw] >> myb) & 1u;
                ns = g.oscore[e0 + f + 1];
                const uint32_t *lr = lk + (int64_t)(f + 1) * R * W;
#pragma unroll
                for (int w = 0; w < kSqMaxW; ++w) if (w < W) nlw[w] = lr[w];
            }
            const int pb = (f & 1) ^ 1, cb = f & 1;
            double b = -1.0, bst = -1.0, mxv = 0.0;
            int p = -1;
            if (cl) {
                if (f > 0) {
#pragma unroll
                    for (int w = 0; w < kSqMaxW; ++w) {
                        if (w >= W) break;
                        uint32_t m = clw[w] & slive[pb][w];
                        while (m) {            // (at most 32 bits)
                            const int q = 32 * w + __builtin_ctz(m);
                            m &= m - 1u;
                            const double bq = sbest[pb][q];
                            if (bq >= 0.0 && (p < 0 || bq > b)) { b = bq; p = q; }
                        }
                    }
                }
                if (p >= 0) {
                    const double pm = smx[pb][p];
                    bst = cs + b;
                    mxv = cs > pm ? cs : pm;
                } else {
                    bst = cs;
                    mxv = cs;
                }
                ptrs[(int64_t)f * Rp + r] = (int16_t)p;
                if (mine.r < 0 || bst > mine.v) mine = SqCand{bst, mxv, f, r};
            }
            sbest[cb][r] = cl ? bst : -1.0;
            smx[cb][r] = mxv;
            const unsigned long long bal = __ballot(cl != 0u);
            if (lane == 0) slive[cb][2 * wv] = (uint32_t)bal;
            if (lane == 32) slive[cb][2 * wv + 1] = (uint32_t)(bal >> 32);
            __syncthreads();
        }
        // ---- end node: wave, then block
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            SqCand x;
            x.v = __shfl_xor(mine.v, o, 64); x.m = __shfl_xor(mine.m, o, 64);
            x.f = __shfl_xor(mine.f, o, 64); x.r = __shfl_xor(mine.r, o, 64);
            if (sq_better(x, mine)) mine = x;
        }
        if (lane == 0) scand[wv] = mine;
        __syncthreads();
        if (r == 0) {
            SqCand top = scand[0];
            for (int i = 1; i < nw; ++i) if (sq_better(scand[i], top)) top = scand[i];
            int go = 0;
            if (top.r < 0) { g.oexh[vc] = 1; g.done[vc] = 1; }
            else if (top.v < g.min_score) { g.done[vc] = 1; }
            else {
                int pf = top.f, pr = top.r, len = 0;
                for (int n = 0; n <= top.f; ++n) {     // (frame 0 has no predecessor: the walk ends there at the latest)
                    path[pf] = (int16_t)pr;
                    ++len;
                    const int q = ptrs[(int64_t)pf * Rp + pr];
                    if (q < 0) break;
                    pr = q;
                    --pf;
                }
                const int64_t i = vc * g.S + k;
                g.oseq_sum[i] = top.v;
                g.oseq_len[i] = len;
                g.oseq_end[2 * i] = top.f;
                g.oseq_end[2 * i + 1] = top.r;
                g.onseq[vc] = k + 1;
                sctl[0] = pf; sctl[1] = top.f;
                snew = g.rescore == 0 ? top.v / (double)len : top.m;
                go = 1;
            }
            sctl[2] = go;
        }
        __syncthreads();
        if (!sctl[2]) return;
        // ---- members and suppression, frame by frame of the path, no barrier
        const int fs = sctl[0], fe = sctl[1];
        const double nv = snew;
        for (int f = fs; f <= fe; ++f) {
            const int p = path[f];
            bool gone = false;
            uint32_t word = 0u;
            if (active) {
                word = lv[(int64_t)f * W + myw];
                const int64_t e = e0 + f;
                if (r == p) {
                    gone = true;
                    g.otracks[e * 5 + 4] = (float)nv;
                    g.oscore[e] = nv;
                    g.oseq[e] = k;
                } else if ((word >> myb) & 1u) {
                    const float4 bp = sq_box(g.tracks + (e + (int64_t)(p - r) * Fv) * 5);
                    const float4 br = sq_box(g.tracks + e * 5);
                    if (sq_hit(bp, br, g.nms_t)) {
                        gone = true;
                        float *o = g.otracks + e * 5;
                        o[0] = qnan; o[1] = qnan; o[2] = qnan; o[3] = qnan; o[4] = qnan;
                        g.oscore[e] = qnan64;
                        g.oseq[e] = kSqSeqSupp;
                    }
                }
            }
            const unsigned long long bal = __ballot(gone);
            const uint32_t mine32 = (lane & 32) ? (uint32_t)(bal >> 32) : (uint32_t)bal;
            if (active && (lane & 31) == 0 && mine32) lv[(int64_t)f * W + myw] = word & ~mine32;
        }
        ++k;
        __syncthreads();
    }
}

}  // namespace vdet
