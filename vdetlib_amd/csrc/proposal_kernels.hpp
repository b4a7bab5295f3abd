// proposal_kernels.hpp -- the proposal layer of a region proposal network on the device (the Faster R-CNN route's boxes):
// anchors, decode, clip, size filter, top-N, NMS, top-N.  THE rule is tests/rpn_spec.py (a restatement of the public
// py-faster-rcnn proposal layer, which was not at hand); the decode is decode_kernels.hpp's decode_box_f64 with the width term
// 1.0 and an optional clamp of dw / dh.
//
// Three kernels of the call's four stages (the NMS in between is the ordered-list NMS of the volume routes, one list per frame):
//   rpn_decode_kernel   one workgroup per (frame, feature row, 64 cells): lanes along w, so the NCHW planes of the score and of
//                       the four deltas are read coalesced; every thread builds its anchor, decodes it, tests validity; keys and
//                       boxes leave in (h,w,a) order through an LDS tile, so the stores are contiguous.  key = the score as a
//                       monotone u32 (-0.0 folded onto +0.0), 0 = not a candidate (no score maps to 0: -inf is 0x007FFFFF)
//   rpn_select_kernel   one workgroup per frame: exact radix select of the pre-th largest (key, index) -- four 8-bit passes over
//                       the key, and only when the cut falls inside a tie class three more over the index --, compaction of the
//                       selection into LDS, bitonic sort by (key desc, index desc) as one u64, then the candidates' boxes, scores,
//                       indices, the identity order list and the count; rows behind the count are NaN / -1
//   rpn_gather_kernel   the first min(survivors, post) kept candidates to the outputs, NaN / -1 behind the count
// Offsets are 64-bit.  The atomics are LDS integer adds (histogram, compaction cursor); (key, index) pairs are unique, so the
// sorted order -- and with it every output -- does not depend on the order the atomics were served in.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "decode_kernels.hpp"

namespace vdet {

constexpr int kRpnMaxA = 64;            // anchors per cell
constexpr int kRpnMaxPre = 16384;       // candidates per frame: 16384 x 8 B of LDS for the sort
constexpr int kRpnAC = 16;              // anchors per LDS tile of the decode pass
constexpr int kRpnSelBlock = 1024;

struct RpnDecodeArgs {
    const float *scores;        // frame f, anchor a, cell (h,w): scores[f*sstride + (a*Hf + h)*Wf + w]
    int64_t sstride;
    const float *deltas;        // [F,4A,Hf,Wf]
    const double *anchors;      // [A,4]
    int A, Hf, Wf, wtiles;      // wtiles = ceil(Wf / 64)
    int64_t N;                  // Hf*Wf*A
    double stride, wmax, hmax, min_size, offset, dw_max;
    int use_dw_max;
    uint32_t *keys;             // [F,N]
    float4 *boxes;              // [F,N]
};

__device__ __forceinline__ uint32_t rpn_key(float s)
{
    if (s != s) return 0u;
    const uint32_t u = __float_as_uint(s == 0.0f ? 0.0f : s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(256) void rpn_decode_kernel(const RpnDecodeArgs g)
{
    __shared__ uint32_t skey[64 * kRpnAC];
    __shared__ float4 sbox[64 * kRpnAC];
    const int64_t blk = blockIdx.x;
    const int wt = (int)(blk % g.wtiles);
    const int64_t fh = blk / g.wtiles;
    const int h = (int)(fh % g.Hf);
    const int64_t f = fh / g.Hf;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int w0 = wt * 64, w = w0 + lane;
    const int wn = g.Wf - w0 < 64 ? g.Wf - w0 : 64;
    const int64_t HW = (int64_t)g.Hf * g.Wf, cell = (int64_t)h * g.Wf + w;
    const float *sc = g.scores + f * g.sstride;
    const float *dl = g.deltas + f * 4 * g.A * HW;
    const int64_t out0 = f * g.N + ((int64_t)h * g.Wf + w0) * g.A;
    const double sx = (double)w * g.stride, sy = (double)h * g.stride;
    for (int a0 = 0; a0 < g.A; a0 += kRpnAC) {
        const int ac = g.A - a0 < kRpnAC ? g.A - a0 : kRpnAC;
        for (int al = wv; al < ac; al += 4) {
            const int a = a0 + al;
            if (lane < wn) {
                const double *an = g.anchors + 4 * a;
                const float s = sc[a * HW + cell];
                const float *d = dl + (int64_t)4 * a * HW + cell;
                double dw = (double)d[2 * HW], dh = (double)d[3 * HW];
                if (g.use_dw_max) {
                    dw = dw > g.dw_max ? g.dw_max : dw;
                    dh = dh > g.dw_max ? g.dw_max : dh;
                }
                const float4 b = decode_box_f64(an[0] + sx, an[1] + sy, an[2] + sx, an[3] + sy, (double)d[0], (double)d[HW], dw, dh,
                                                g.wmax, g.hmax, g.offset);
                const bool ok = ((double)b.z - (double)b.x) + 1.0 >= g.min_size && ((double)b.w - (double)b.y) + 1.0 >= g.min_size;
                skey[lane * ac + al] = ok ? rpn_key(s) : 0u;
                sbox[lane * ac + al] = b;
            }
        }
        __syncthreads();
        const int n = wn * ac;
        for (int i = threadIdx.x; i < n; i += 256) {
            const int wl = i / ac, al = i - wl * ac;
            const int64_t o = out0 + (int64_t)wl * g.A + a0 + al;
            g.keys[o] = skey[i];
            g.boxes[o] = sbox[i];
        }
        __syncthreads();
    }
}

struct RpnSelectArgs {
    const uint32_t *keys;       // [F,N]
    const float4 *boxes;        // [F,N]
    const float *scores;
    int64_t sstride;
    int A;
    int64_t HW, N;
    int pre, p2;                // p2 = the power of two >= pre: the u64 entries of the dynamic LDS
    float4 *cand_boxes;         // [F,pre]
    float *cand_scores;         // [F,pre]
    int32_t *cand_index;        // [F,pre]
    uint16_t *order;            // [F,pre]: 0 .. pre-1, the list the ordered NMS walks
    int32_t *cand_cnt;          // [F]
};

// one digit of the radix select, called by every thread of the block once hist[] holds the digit's histogram over the elements
// still in the running: res[0] the digit that holds the want-th largest, res[1] the count of larger digits, res[2] the count of
// that digit, res[3] the histogram's sum
__device__ __forceinline__ void rpn_pick_digit(uint32_t *hist, uint32_t *res, uint32_t want)
{
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t above = 0, d = 0, at = 0, total = 0;
        bool found = false;      // (the callers ask for want <= the histogram's sum)
        for (int b = 255; b >= 0; --b) {
            const uint32_t hcnt = hist[b];
            total += hcnt;
            if (!found) {
                if (above + hcnt >= want) { d = (uint32_t)b; at = hcnt; found = true; }
                else above += hcnt;
            }
        }
        res[0] = d; res[1] = above; res[2] = at; res[3] = total;
    }
    __syncthreads();
}

__global__ __launch_bounds__(kRpnSelBlock) void rpn_select_kernel(const RpnSelectArgs g)
{
    extern __shared__ unsigned long long rpn_sort[];      // [p2]
    __shared__ uint32_t hist[256];
    __shared__ uint32_t res[8];
    __shared__ uint32_t cursor;
    const int64_t f = blockIdx.x;
    const int tid = threadIdx.x;
    const uint32_t *keys = g.keys + f * g.N;
    const uint32_t N = (uint32_t)g.N;

    // ---- the pre-th largest key T, and how many of the keys equal to T are taken
    uint32_t prefix = 0, mask = 0, want = (uint32_t)g.pre, at = 0;
    bool all = false;
    for (int pass = 0; pass < 4 && !all; ++pass) {
        const int shift = 24 - 8 * pass;
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        for (uint32_t i = tid; i < N; i += kRpnSelBlock) {
            const uint32_t k = keys[i];
            if (k != 0u && (k & mask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1u);
        }
        rpn_pick_digit(hist, res, want);
        if (pass == 0 && res[3] <= (uint32_t)g.pre) { all = true; break; }      // fewer candidates than pre: all of them
        prefix |= res[0] << shift;
        mask |= 255u << shift;
        want -= res[1];
        at = res[2];
    }
    // all: every nonzero key (the smallest one is 0x007FFFFF, -inf); else key > T, and of key == T the `want` highest indices
    uint32_t T = all ? 1u : prefix, idx_min = 0;
    if (!all && want < at) {
        uint32_t ipre = 0, imask = 0;
        for (int pass = 0; pass < 3; ++pass) {
            const int shift = 16 - 8 * pass;
            if (tid < 256) hist[tid] = 0;
            __syncthreads();
            for (uint32_t i = tid; i < N; i += kRpnSelBlock)
                if (keys[i] == T && (i & imask) == ipre) atomicAdd(&hist[(i >> shift) & 255u], 1u);
            rpn_pick_digit(hist, res, want);
            ipre |= res[0] << shift;
            imask |= 255u << shift;
            want -= res[1];
        }
        idx_min = ipre;
    }

    // ---- compaction into LDS (any order: the pairs are unique and sorted next)
    if (tid == 0) cursor = 0;
    __syncthreads();
    const uint32_t rounds = (N + kRpnSelBlock - 1) / kRpnSelBlock;
    for (uint32_t r = 0; r < rounds; ++r) {
        const uint32_t i = r * kRpnSelBlock + tid;
        const uint32_t k = i < N ? keys[i] : 0u;
        const bool take = k != 0u && (k > T || (k == T && (all || i >= idx_min)));
        const unsigned long long m = __ballot(take);
        uint32_t base = 0;
        if ((tid & 63) == 0 && m) base = atomicAdd(&cursor, (uint32_t)__popcll(m));
        base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
        if (take) {
            const uint32_t pos = base + (uint32_t)__popcll(m & ((1ull << (tid & 63)) - 1ull));
            if (pos < (uint32_t)g.p2) rpn_sort[pos] = ((unsigned long long)k << 32) | i;
        }
    }
    __syncthreads();
    uint32_t M = cursor;
    M = M < (uint32_t)g.pre ? M : (uint32_t)g.pre;
    uint32_t n2 = 1;
    while (n2 < M) n2 <<= 1;
    for (uint32_t i = M + tid; i < n2; i += kRpnSelBlock) rpn_sort[i] = 0ull;
    __syncthreads();

    // ---- bitonic sort, descending (the zero padding goes last)
    for (uint32_t k = 2; k <= n2; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t p = tid; p < (n2 >> 1); p += kRpnSelBlock) {
                const uint32_t lo = ((p & ~(j - 1)) << 1) | (p & (j - 1)), hi = lo | j;
                const unsigned long long a = rpn_sort[lo], b = rpn_sort[hi];
                const bool desc = (lo & k) == 0;
                if (desc ? a < b : a > b) { rpn_sort[lo] = b; rpn_sort[hi] = a; }
            }
            __syncthreads();
        }
    }

    // ---- the candidates in order
    const float nanf = __builtin_nanf("");
    const int64_t o0 = f * g.pre;
    for (uint32_t r = tid; r < (uint32_t)g.pre; r += kRpnSelBlock) {
        float4 b = make_float4(nanf, nanf, nanf, nanf);
        float s = nanf;
        int32_t idx = -1;
        if (r < M) {
            const uint32_t i = (uint32_t)rpn_sort[r];
            if (i < N) {
                idx = (int32_t)i;
                b = g.boxes[f * g.N + i];
                const uint32_t cell = i / (uint32_t)g.A, a = i - cell * (uint32_t)g.A;
                s = g.scores[f * g.sstride + (int64_t)a * g.HW + cell];
            }
        }
        g.cand_boxes[o0 + r] = b;
        g.cand_scores[o0 + r] = s;
        g.cand_index[o0 + r] = idx;
        g.order[o0 + r] = (uint16_t)r;
    }
    if (tid == 0) g.cand_cnt[f] = (int32_t)M;
}

struct RpnGatherArgs {
    const float4 *cand_boxes;   // [F,pre]
    const float *cand_scores;
    const int32_t *cand_index;
    const int32_t *keep;        // [F,pre] positions among the candidates, in order
    const int32_t *keep_cnt;    // [F]
    int64_t F;
    int pre, post;
    float4 *rois;               // [F,post]
    float *scores;
    int32_t *index;
    int32_t *count;             // [F]
};

__global__ __launch_bounds__(256) void rpn_gather_kernel(const RpnGatherArgs g)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= g.F * g.post) return;
    const int64_t f = i / g.post;
    const int r = (int)(i - f * g.post);
    int n = g.keep_cnt[f];
    n = n < 0 ? 0 : (n < g.post ? n : g.post);
    const float nanf = __builtin_nanf("");
    float4 b = make_float4(nanf, nanf, nanf, nanf);
    float s = nanf;
    int32_t idx = -1;
    if (r < n) {
        const int k = g.keep[f * g.pre + r];
        if (k >= 0 && k < g.pre) {
            const int64_t e = f * g.pre + k;
            b = g.cand_boxes[e]; s = g.cand_scores[e]; idx = g.cand_index[e];
        }
    }
    g.rois[i] = b;
    g.scores[i] = s;
    g.index[i] = idx;
    if (r == 0) g.count[f] = n;
}

}  // namespace vdet
