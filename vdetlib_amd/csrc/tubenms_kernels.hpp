// NMS over whole tubelets by spatio-temporal overlap (include/vdet_hip.h: vdet_nms_tubelets; the rule once more in numpy:
// tests/tubenms_spec.py).  The reference has no such function: the rule is the project's own, and every result is defined as
// an integer or as ONE IEEE operation on integers, so that the device equals the numpy statement on bits.
//
// A PROBLEM is one (video, class): T <= 256 tubelet slots over the video's F frames.  Four launches, no host wait between them:
//   1. tubenms_score_kernel   one wave per (problem, slot): n (boxes), the frame extent [first, last] and the tubelet score ts
//                             (f64).  'mean' is DEFINED as the sum in ascending frame order, so the wave loads 64 frames at a
//                             time (coalesced) and adds the valid lanes' values one after the other, every lane the same sum.
//                             ts is NaN for an ABSENT slot (no box, a NaN score, t >= ntracks): that NaN is the present flag
//                             of every later launch.
//   2. tubenms_pair_kernel    the hot part.  Grid (upper-triangle TILES of 32 x 32 slot pairs x classes, videos): the tile axis
//                             is what fills the chip when there are fewer problems than CUs.  A workgroup of 256 threads owns
//                             its 1024 pairs over ALL frames, four pairs per thread (one column slot, four row slots) with the
//                             integer sum S (u64) and the shared-frame count I in registers -- so no atomics at all.  Frames
//                             are staged in chunks of kTubeFC = 32 through LDS as 16-byte rows laid out [frame][64 slots] (pitch
//                             65 rows: the staging stores of one 8-lane group land on distinct banks; the reads are one
//                             contiguous run per 32 lanes for the column slot and a broadcast for the row slot).  tboxes come
//                             in as one 16-byte load per box, tracks rows (20 bytes, no alignment) as four dwords.  Existence
//                             travels beside the boxes as one 32-bit ballot word per (slot, chunk): I is a popcount per chunk,
//                             and the frame loop visits only the frames on which some row slot AND some column slot have a
//                             box.  Chunks outside the intersection of the tile's row extent and column extent are never
//                             loaded (tubelets disjoint in time cost nothing); tiles behind ntracks exit at once.
//                             Per pair the overlap is one f64 division; what leaves the kernel is the BIT ovr >= thresh, a
//                             T x ceil(T/32) word matrix per problem (8 KB at T = 256), both halves: the tile transposes its
//                             32 ballot words through LDS.  The f64 matrix is written only when the caller asks for it.
//   3. tubenms_select_kernel  one wave per problem: rank by (ts, slot) with T*T/64 compares per lane, bit rows and order in
//                             LDS, then the greedy walk with the decided set as one word per lane.
//   4. tubenms_gather_kernel  one wave per OUTPUT slot: the merge kernel's ragged copy (merge_kernels.hpp) of slot src[r] into
//                             rank r, NaN rows / zero anchors behind the count.
// Selection is not fused into the pair pass: a last-block-done scheme would put a device-wide counter and a fence on the hot
// kernel to save one launch of a few microseconds.
// No float atomics on any result path (there are no atomics at all); no status bit: nothing here is an error on the device.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "batch_kernels.hpp"     // VidDesc
#include "merge_kernels.hpp"     // wave_copy_words, wave_fill_words, kMergeMaxSeries
#include "nms_kernels.hpp"       // ref_max, ref_min

namespace vdet {

constexpr int kTubeMaxT = 256;
constexpr int kTubeTile = 32;               // slots per tile side
constexpr int kTubeFC = 32;                 // frames per staged chunk (tests/test_tubenms_gpu.py: CHUNK)
constexpr int kTubePitch = 2 * kTubeTile + 1;   // 16-byte rows per staged frame
constexpr int kTubeLT = 256;
constexpr int kTubeWaves = kTubeLT / 64;
constexpr int kTubeNormUnion = 0, kTubeNormShared = 1, kTubeNormMin = 2;
constexpr int kTubeScoreSlot = 0, kTubeScoreMean = 1, kTubeScoreMax = 2;

// per problem p = v*C + c, in the context's scratch
struct TubeScratch {
    double *ts;          // [P,T]   NaN: absent
    int32_t *n;          // [P,T]
    int32_t *first;      // [P,T]   (F, -1 for a slot without a box)
    int32_t *last;       // [P,T]
    uint32_t *bits;      // [P,T,W] bit u of word w of row t: ovr(t, 32w + u) >= thresh
};

struct TubeArgs {
    const float *tracks;        // [C,T,F,5]  (batch: video v at element C*T*5*f0)
    const int32_t *ntracks;     // [V,C]
    const float *tboxes;        // [C,T,F,4] or null
    const void *score;          // [V,C,T] (mode 0) or [C,T,F]
    const float *anchors;       // [V,C,T,3] or null
    const double *series[kMergeMaxSeries];
    const VidDesc *vids;        // null: one video of F frames
    int F, C, T, W, nser;
    int score_f64, score_mode, norm, min_shared;
    double thresh;
    TubeScratch s;
    float *otracks;
    int32_t *ontracks;          // [V,C]
    float *oanchors;
    float *otboxes;
    double *oseries;            // [nser][oN]
    int64_t oN;                 // C*T*(all frames)
    int32_t *src;               // [V,C,T]
    double *tscore;             // [V,C,T]
    int32_t *by;                // [V,C,T]
    double *overlaps;           // [V,C,T,T] or null
};

struct TubeVid { int64_t f0; int F; };

__device__ __forceinline__ TubeVid tube_video(const TubeArgs &g, int v)
{
    TubeVid m{0, g.F};
    if (g.vids) { const VidDesc vd = g.vids[v]; m.f0 = vd.f0; m.F = vd.F; }
    return m;
}

__device__ __forceinline__ int tube_count(const TubeArgs &g, int64_t p)
{
    const int n = g.ntracks[p];
    return n < 0 ? 0 : (n > g.T ? g.T : n);
}

// first element of slot (c, t) of the video's [C,T,F_v] block
__device__ __forceinline__ int64_t tube_elem(const TubeArgs &g, const TubeVid &m, int c, int t)
{
    return (int64_t)g.C * g.T * m.f0 + ((int64_t)c * g.T + t) * m.F;
}

// a total order on doubles that are not NaN, -0.0 below +0.0: what makes 'max' independent of the order of the frames
__device__ __forceinline__ int64_t tube_order_key(double x)
{
    const int64_t b = __double_as_longlong(x);
    return b ^ ((b >> 63) & 0x7FFFFFFFFFFFFFFFll);
}

__global__ __launch_bounds__(kTubeLT) void tubenms_score_kernel(const TubeArgs g)
{
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t s = (int64_t)blockIdx.x * kTubeWaves + w;
    if (s >= (int64_t)g.C * g.T) return;
    const int v = blockIdx.y, c = (int)(s / g.T), t = (int)(s - (int64_t)c * g.T);
    const TubeVid m = tube_video(g, v);
    const int64_t p = (int64_t)v * g.C + c, slot = p * g.T + t;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    int n = 0, first = m.F, last = -1;
    double ts = nan;
    if (t < tube_count(g, p)) {
        const int64_t e = tube_elem(g, m, c, t);
        double sum = 0.0;
        int cnt = 0;
        int64_t best = INT64_MIN;
        for (int base = 0; base < m.F; base += 64) {
            const int f = base + lane;
            bool ex = false, ok = false;
            double val = nan;
            if (f < m.F) {
                const float x = g.tracks[(e + f) * 5];
                ex = !(x != x);
                if (ex && g.score_mode != kTubeScoreSlot) {
                    val = g.score_f64 ? static_cast<const double *>(g.score)[e + f] : (double)static_cast<const float *>(g.score)[e + f];
                    ok = !(val != val);
                }
            }
            const unsigned long long me = __ballot(ex);
            if (me) {
                if (first == m.F) first = base + (int)__builtin_ctzll(me);
                last = base + 63 - (int)__builtin_clzll(me);
                n += __popcll(me);
            }
            if (g.score_mode == kTubeScoreMean) {
                for (unsigned long long mv = __ballot(ok); mv; mv &= mv - 1ull) {     // ascending frame order: the definition
                    sum += __shfl(val, (int)__builtin_ctzll(mv));
                    ++cnt;
                }
            } else if (g.score_mode == kTubeScoreMax && ok) {
                const int64_t k = tube_order_key(val);
                best = k > best ? k : best;
                ++cnt;
            }
        }
        if (g.score_mode == kTubeScoreSlot) {
            if (n > 0) ts = g.score_f64 ? static_cast<const double *>(g.score)[slot] : (double)static_cast<const float *>(g.score)[slot];
        } else if (g.score_mode == kTubeScoreMean) {
            if (cnt > 0) ts = sum / (double)cnt;
        } else {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                const int64_t o = __shfl_xor(best, d);
                best = o > best ? o : best;
                cnt += __shfl_xor(cnt, d);
            }
            if (cnt > 0) ts = __longlong_as_double(best ^ ((best >> 63) & 0x7FFFFFFFFFFFFFFFll));
        }
    }
    if (lane == 0) {
        g.s.ts[slot] = ts; g.s.n[slot] = n; g.s.first[slot] = first; g.s.last[slot] = last;
    }
}

// the frame's contribution: rint(q * 2^24) for a finite q > 0, saturated at 2^32 - 1; 0 for every other q
__device__ __forceinline__ uint32_t tube_quant(float4 a, float4 b)
{
    const float aarea = ((a.z - a.x) + 1.0f) * ((a.w - a.y) + 1.0f);
    const float barea = ((b.z - b.x) + 1.0f) * ((b.w - b.y) + 1.0f);
    const float xx1 = ref_max(a.x, b.x);
    const float yy1 = ref_max(a.y, b.y);
    const float xx2 = ref_min(a.z, b.z);
    const float yy2 = ref_min(a.w, b.w);
    const float w = ref_max(0.0f, (xx2 - xx1) + 1.0f);
    const float h = ref_max(0.0f, (yy2 - yy1) + 1.0f);
    const float inter = w * h;
    const float q = inter / ((aarea + barea) - inter);
    if (!(q > 0.0f && q <= 3.4028234663852886e38f)) return 0u;
    const float r = __builtin_rintf(q * 16777216.0f);
    return r >= 4294967296.0f ? 0xFFFFFFFFu : (uint32_t)r;
}

__global__ __launch_bounds__(kTubeLT) void tubenms_pair_kernel(const TubeArgs g)
{
    __shared__ __attribute__((aligned(16))) float4 sbox[kTubeFC * kTubePitch];     // [frame][row slots 0..31 | column slots 32..63]
    __shared__ uint32_t sex[2 * kTubeTile];         // existence of the chunk's frames per staged slot
    __shared__ uint32_t sbits[kTubeTile];
    __shared__ int sn[2 * kTubeTile], sfirst[2 * kTubeTile], slast[2 * kTubeTile];
    __shared__ uint32_t spresent[2];
    const int tid = threadIdx.x, lane = tid & 63;
    const int nt1 = (g.T + kTubeTile - 1) / kTubeTile, ntiles = nt1 * (nt1 + 1) / 2;
    const int c = blockIdx.x / ntiles, v = blockIdx.y;
    int ta = 0, tb = blockIdx.x - c * ntiles;       // tile (ta, tb), ta <= tb: row ta holds nt1 - ta tiles
    while (tb >= nt1 - ta) { tb -= nt1 - ta; ++ta; }
    tb += ta;
    const int64_t p = (int64_t)v * g.C + c;
    const int nt = tube_count(g, p);
    if (!g.overlaps && tb * kTubeTile >= nt) return;            // no present pair, and no word of the tile is ever read
    const TubeVid m = tube_video(g, v);
    const float qnan = __uint_as_float(0x7FC00000u);

    // the tile's 64 slots: counts, extents, presence
    if (tid < 2 * kTubeTile) {
        const int t = (tid < kTubeTile ? ta : tb) * kTubeTile + (tid & (kTubeTile - 1));
        int n = 0, first = m.F, last = -1;
        bool present = false;
        if (t < nt) {
            const int64_t slot = p * g.T + t;
            const double ts = g.s.ts[slot];
            present = !(ts != ts);
            n = g.s.n[slot]; first = g.s.first[slot]; last = g.s.last[slot];
        }
        sn[tid] = n; sfirst[tid] = first; slast[tid] = last;
        const unsigned long long pm = __ballot(present);
        if (lane == 0) { spresent[0] = (uint32_t)pm; spresent[1] = (uint32_t)(pm >> 32); }
    }
    __syncthreads();
    // frames on which a row slot and a column slot can both have a box
    int lo, hi;
    {
        int alo = m.F, ahi = -1, blo = m.F, bhi = -1;
        for (int i = 0; i < kTubeTile; ++i) {
            alo = min(alo, sfirst[i]); ahi = max(ahi, slast[i]);
            blo = min(blo, sfirst[kTubeTile + i]); bhi = max(bhi, slast[kTubeTile + i]);
        }
        lo = max(alo, blo); hi = min(ahi, bhi);
    }
    const int j = tid & (kTubeTile - 1), i0 = tid >> 5;        // column slot j, row slots i0 + 8k
    unsigned long long S[4] = {0ull, 0ull, 0ull, 0ull};
    int I[4] = {0, 0, 0, 0};
    const bool tb16 = g.tboxes && (reinterpret_cast<uintptr_t>(g.tboxes) & 15) == 0;
    for (int base = lo >= 0 ? (lo / kTubeFC) * kTubeFC : 0; base <= hi; base += kTubeFC) {
        // stage: thread -> frame tid & 31 of staged slots (tid >> 5) + 8r
        const int f = base + (tid & (kTubeFC - 1));
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int ss = (tid >> 5) + 8 * r;
            const int t = (ss < kTubeTile ? ta : tb) * kTubeTile + (ss & (kTubeTile - 1));
            float4 b = make_float4(qnan, qnan, qnan, qnan);
            bool ex = false;
            if (t < nt && f < m.F && f >= sfirst[ss] && f <= slast[ss]) {
                const int64_t e = tube_elem(g, m, c, t) + f;
                const float *row = g.tracks + e * 5;
                const float x = row[0];
                ex = !(x != x);
                if (ex) {
                    if (tb16) b = *reinterpret_cast<const float4 *>(g.tboxes + e * 4);
                    else if (g.tboxes) { const float *q = g.tboxes + e * 4; b = make_float4(q[0], q[1], q[2], q[3]); }
                    else b = make_float4(x, row[1], row[2], row[3]);
                }
            }
            sbox[(tid & (kTubeFC - 1)) * kTubePitch + ss] = b;
            const unsigned long long me = __ballot(ex);
            if ((tid & 31) == 0) sex[ss] = (lane & 32) ? (uint32_t)(me >> 32) : (uint32_t)me;
        }
        __syncthreads();
        uint32_t aany = 0, bany = 0;
        for (int i = 0; i < kTubeTile; ++i) { aany |= sex[i]; bany |= sex[kTubeTile + i]; }
        const uint32_t eb = sex[kTubeTile + j];
        uint32_t meet[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            meet[k] = sex[i0 + 8 * k] & eb;
            I[k] += __popc(meet[k]);
        }
        for (uint32_t fm = aany & bany; fm; fm &= fm - 1u) {        // (uniform over the workgroup)
            const int ff = __builtin_ctz(fm);
            const float4 b = sbox[ff * kTubePitch + kTubeTile + j];
#pragma unroll
            for (int k = 0; k < 4; ++k)         // a wave none of whose 64 pairs shares the frame skips the arithmetic (a missing box is a NaN row: 0 anyway)
                if (__any((meet[k] >> ff) & 1u)) S[k] += tube_quant(sbox[ff * kTubePitch + i0 + 8 * k], b);
        }
        __syncthreads();
    }

    // the pairs' overlaps, their bits, and both halves of the bit matrix
    const int tj = tb * kTubeTile + j, nj = sn[kTubeTile + j];
    const bool pj = (spresent[1] >> j) & 1u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = i0 + 8 * k, ti = ta * kTubeTile + i, ni = sn[i];
        const bool mine = ta < tb || i <= j;                    // the diagonal tile: the upper triangle only
        const bool both = mine && ((spresent[0] >> i) & 1u) && pj;
        double ovr = 0.0;
        if (both) {
            const int den = g.norm == kTubeNormUnion ? ni + nj - I[k] : g.norm == kTubeNormShared ? I[k] : min(ni, nj);
            if (den != 0 && I[k] >= g.min_shared) ovr = (double)S[k] / ((double)den * 16777216.0);
        }
        const unsigned long long hit = __ballot(both && ovr >= g.thresh);
        if ((tid & 31) == 0) sbits[i] = (lane & 32) ? (uint32_t)(hit >> 32) : (uint32_t)hit;
        if (g.overlaps && mine && ti < g.T && tj < g.T) {
            const double o = both ? ovr : __longlong_as_double(0x7FF8000000000000ll);
            double *ov = g.overlaps + p * g.T * g.T;
            ov[(int64_t)ti * g.T + tj] = o;
            ov[(int64_t)tj * g.T + ti] = o;
        }
    }
    __syncthreads();
    if (tid < kTubeTile) {
        uint32_t tw = 0;
        for (int i = 0; i < kTubeTile; ++i) tw |= ((sbits[i] >> tid) & 1u) << i;
        uint32_t *bits = g.s.bits + p * g.T * g.W;
        const int ra = ta * kTubeTile + tid, rb = tb * kTubeTile + tid;
        if (ta == tb) {
            if (ra < g.T) bits[(int64_t)ra * g.W + ta] = sbits[tid] | tw;
        } else {
            if (ra < g.T) bits[(int64_t)ra * g.W + tb] = sbits[tid];
            if (rb < g.T) bits[(int64_t)rb * g.W + ta] = tw;
        }
    }
}

__global__ __launch_bounds__(64) void tubenms_select_kernel(const TubeArgs g)
{
    __shared__ double sts[kTubeMaxT];
    __shared__ uint32_t srow[kTubeMaxT * (kTubeMaxT / 32)];
    __shared__ int sorder[kTubeMaxT], sby[kTubeMaxT], skept[kTubeMaxT];
    const int lane = threadIdx.x;
    const int64_t p = blockIdx.x;
    const int T = g.T, W = g.W;
    const int nt = tube_count(g, p), Wn = (nt + 31) >> 5;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    for (int t = lane; t < T; t += 64) {
        sts[t] = t < nt ? g.s.ts[p * T + t] : nan;
        sby[t] = -1;
    }
    for (int x = lane; x < nt * Wn; x += 64) {          // the rows and words of slots below ntracks: all that the pair pass wrote
        const int t = x / Wn, w = x - t * Wn;
        srow[t * W + w] = g.s.bits[(p * T + t) * W + w];
    }
    __syncthreads();
    // rank: the number of present slots in front of t
    int np = 0;
    for (int t = lane; t < nt; t += 64) {
        const double x = sts[t];
        if (x != x) continue;
        int r = 0;
        for (int u = 0; u < nt; ++u) {
            const double y = sts[u];
            r += (y > x || (y == x && u > t)) ? 1 : 0;
        }
        sorder[r] = t;
        ++np;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) np += __shfl_xor(np, d);
    __syncthreads();
    // lane w < W holds word w of the decided set: absent slots are decided from the start
    uint32_t done = 0;
    if (lane < W)
        for (int u = 0; u < 32; ++u) {
            const int t = lane * 32 + u;
            const double x = t < nt ? sts[t] : nan;
            if (x != x) done |= 1u << u;
        }
    int nk = 0;
    for (int r = 0; r < np; ++r) {
        const int t = sorder[r];
        const uint32_t dw = __shfl(done, t >> 5);
        if ((dw >> (t & 31)) & 1u) continue;            // suppressed by a kept tubelet in front of it
        if (lane == 0) { skept[nk] = t; sby[t] = t; }
        ++nk;
        if (lane < W) {
            if (lane == (t >> 5)) done |= 1u << (t & 31);
            uint32_t fresh = srow[t * W + lane] & ~done;
            done |= fresh;
            for (; fresh; fresh &= fresh - 1u) sby[lane * 32 + __builtin_ctz(fresh)] = t;
        }
    }
    __syncthreads();
    if (lane == 0) g.ontracks[p] = nk;
    for (int r = lane; r < T; r += 64) {
        const int t = r < nk ? skept[r] : 0;
        g.src[p * T + r] = r < nk ? t : INT32_MIN;
        g.tscore[p * T + r] = r < nk ? sts[t] : nan;
        g.by[p * T + r] = sby[r];
    }
}

__global__ __launch_bounds__(kTubeLT) void tubenms_gather_kernel(const TubeArgs g)
{
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t s = (int64_t)blockIdx.x * kTubeWaves + w;
    if (s >= (int64_t)g.C * g.T) return;
    const int v = blockIdx.y, c = (int)(s / g.T), r = (int)(s - (int64_t)c * g.T);
    const TubeVid m = tube_video(g, v);
    const int64_t p = (int64_t)v * g.C + c;
    const int t = g.src[p * g.T + r];
    const int64_t oe = tube_elem(g, m, c, r), oslot = p * g.T + r;
    const int64_t F = m.F;
    if (t >= 0 && t < g.T) {
        const int64_t se = tube_elem(g, m, c, t), sslot = p * g.T + t;
        wave_copy_words(reinterpret_cast<uint32_t *>(g.otracks + oe * 5), reinterpret_cast<const uint32_t *>(g.tracks + se * 5), F * 5, lane);
        if (g.otboxes)
            wave_copy_words(reinterpret_cast<uint32_t *>(g.otboxes + oe * 4), reinterpret_cast<const uint32_t *>(g.tboxes + se * 4), F * 4, lane);
#pragma unroll
        for (int q = 0; q < kMergeMaxSeries; ++q)
            if (q < g.nser)
                wave_copy_words(reinterpret_cast<uint32_t *>(g.oseries + q * g.oN + oe), reinterpret_cast<const uint32_t *>(g.series[q] + se),
                                F * 2, lane);
        if (g.oanchors && lane < 3) g.oanchors[oslot * 3 + lane] = g.anchors[sslot * 3 + lane];
    } else {
        const uint32_t qnan = 0x7FC00000u;
        wave_fill_words(reinterpret_cast<uint32_t *>(g.otracks + oe * 5), F * 5, qnan, qnan, lane);
        if (g.otboxes) wave_fill_words(reinterpret_cast<uint32_t *>(g.otboxes + oe * 4), F * 4, qnan, qnan, lane);
#pragma unroll
        for (int q = 0; q < kMergeMaxSeries; ++q)
            if (q < g.nser) wave_fill_words(reinterpret_cast<uint32_t *>(g.oseries + q * g.oN + oe), F * 2, 0u, 0x7FF80000u, lane);
        if (g.oanchors && lane < 3) g.oanchors[oslot * 3 + lane] = 0.0f;
    }
}

}  // namespace vdet
