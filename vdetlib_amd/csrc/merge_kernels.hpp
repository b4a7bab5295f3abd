// Device merge of two scored tubelet sets: the array form of merge_score_protos (reference utils/protocol.py:504-525), in the
// [C,T,F,...] layout every other device stage reads and writes.
//
// A SET is tracks [C,T,F,5] f32, ntracks [C] i32, anchors [C,T,3] f32, optionally tboxes [C,T,F,4] f32, and 1..4 series
// [C,T,F] f64 (series 0 = det_score).  A box exists where tracks[c,t,f,0] is not NaN and t < ntracks[c].  The two sets share
// C, F, the number of series and the presence of tboxes; Ta and Tb may differ.  Counts outside 0..T are clamped.
//
// COMBINE (list extend): out slot t < nta[c] is a's slot t, out slot nta[c] + u (u < ntb[c]) is b's slot u, every slot behind
// is NaN rows / tboxes / series and a zero anchor.  A ragged gather-copy: a slot's rows, tboxes and every series are each one
// contiguous run, moved as 32-bit words -- 16 bytes per lane where source and destination sit at the same offset inside a
// 16-byte line (a scalar head up to the line, a scalar tail behind the last whole line), word by word where they do not.
// F*5*4 bytes per slot is no multiple of 16 for most F, so both paths run in one call.
//
// MAX (zip over the tubelet lists, zip over the box lists): slot t < min(nta[c], ntb[c]) is PAIRED.  With ca / cb boxes on the
// two sides and m = min(ca, cb), the i-th box of a meets the i-th box of b for i < m; they must lie on the same frame and the
// integer anchor frames of the two slots must be equal (m >= 1), else the slot latches kStBadMerge and is written as a copy
// of a.  Where det_b > det_a (f64; a NaN on either side, equal scores and -0.0 against +0.0 keep a) the box takes b's row,
// tboxes and every series; from_b marks it.  Boxes of ordinal >= m, unpaired slots and the anchors are a's.
//   Sweep 1 (ballots over the frames in chunks of 64): ca, cb, and k0 = the number of boxes in front of the first frame that
//   only ONE side has a box on.  The pairing holds for every ordinal < m exactly when k0 >= m: up to that frame the two sides
//   have their boxes on the same frames, and on it the box of ordinal k0 of one side faces a gap of the other.
//   Sweep 2 carries a's running ordinal, compares and writes every element of the slot once.
// The 20-byte rows are NOT staged through LDS.  The existence test reads column 0 strided per lane (one dword at a 20-byte lane
// stride: the lines it pulls in are the ones the move needs next); the move itself treats a chunk's rows as one run of 320
// words and the chunk's verdicts as a 64-bit ballot, so loads and stores are coalesced dwords and no LDS or barrier is needed.
//
// Shape of both kernels: ONE launch, one WAVE per output slot (four per workgroup), grid (ceil(C*T/4), V).  The video's block
// offsets are C*T*f0 with the set's OWN T (Ta, Tb, T_out differ under COMBINE).  No LDS, no atomics on a result path (the
// status word is one atomicOr on the error path), no scratch of the context.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "batch_kernels.hpp"     // VidDesc

namespace vdet {

constexpr int kStBadMerge = 256;     // 'max': a paired slot whose boxes do not pair up frame by frame, or whose anchor frames differ
constexpr int kMergeLT = 256;
constexpr int kMergeWaves = kMergeLT / 64;
constexpr int kMergeMaxSeries = 4;

struct MergeSet {
    const float *tracks;                        // [C,T,F,5]  (batch: video v at element C*T*5*f0)
    const int32_t *ntracks;                     // [V,C]
    const float *anchors;                       // [V,C,T,3]
    const float *tboxes;                        // [C,T,F,4] or null
    const double *series[kMergeMaxSeries];      // [C,T,F]
    int T;
};

struct MergeArgs {
    MergeSet a, b;
    const VidDesc *vids;        // null: one video of F frames
    int F, C, nser, To;         // To: slots per class of the output
    float *otracks;
    int32_t *ontracks;
    float *oanchors;
    float *otboxes;             // null without tboxes
    double *oseries;            // [nser][oN]
    int64_t oN;                 // C*To*(all frames)
    uint8_t *from_b;            // [C,Ta,F] ('max')
    int *status;
};

// n 32-bit words from src to dst by one wave, bit for bit
__device__ __forceinline__ void wave_copy_words(uint32_t *dst, const uint32_t *src, int64_t n, int lane)
{
    const uintptr_t d = (uintptr_t)dst, s = (uintptr_t)src;
    int64_t head = n, nvec = 0;     // (relative misalignment: every word goes one by one)
    if (((d ^ s) & 15) == 0) {
        head = (int64_t)(((16 - (d & 15)) & 15) >> 2);
        head = head < n ? head : n;
        nvec = (n - head) >> 2;
    }
    for (int64_t i = lane; i < head; i += 64) dst[i] = src[i];
    const uint4 *s4 = reinterpret_cast<const uint4 *>(src + head);
    uint4 *d4 = reinterpret_cast<uint4 *>(dst + head);
    int64_t i = lane;
    for (; i + 192 < nvec; i += 256) {      // four loads in flight per lane before the first store
        const uint4 v0 = s4[i], v1 = s4[i + 64], v2 = s4[i + 128], v3 = s4[i + 192];
        d4[i] = v0; d4[i + 64] = v1; d4[i + 128] = v2; d4[i + 192] = v3;
    }
    for (; i < nvec; i += 64) d4[i] = s4[i];
    for (i = head + 4 * nvec + lane; i + 192 < n; i += 256) {
        const uint32_t v0 = src[i], v1 = src[i + 64], v2 = src[i + 128], v3 = src[i + 192];
        dst[i] = v0; dst[i + 64] = v1; dst[i + 128] = v2; dst[i + 192] = v3;
    }
    for (; i < n; i += 64) dst[i] = src[i];
}

// n words at dst: word i = (i odd ? w1 : w0).  An f64 pattern needs dst 8-byte aligned (the head is then 0 or 2 words).
__device__ __forceinline__ void wave_fill_words(uint32_t *dst, int64_t n, uint32_t w0, uint32_t w1, int lane)
{
    int64_t head = (int64_t)(((16 - ((uintptr_t)dst & 15)) & 15) >> 2);
    head = head < n ? head : n;
    const int64_t nvec = (n - head) >> 2;
    for (int64_t i = lane; i < head; i += 64) dst[i] = (i & 1) ? w1 : w0;
    uint4 *d4 = reinterpret_cast<uint4 *>(dst + head);
    const uint4 pat = (head & 1) ? make_uint4(w1, w0, w1, w0) : make_uint4(w0, w1, w0, w1);
    for (int64_t i = lane; i < nvec; i += 64) d4[i] = pat;
    for (int64_t i = head + 4 * nvec + lane; i < n; i += 64) dst[i] = (i & 1) ? w1 : w0;
}

struct MergeSlot { int v, c, t, F; int64_t f0; };

// the wave's output slot; false for the waves behind the last one
__device__ __forceinline__ bool merge_slot(const MergeArgs &g, MergeSlot &m)
{
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t s = (int64_t)blockIdx.x * kMergeWaves + w;
    if (s >= (int64_t)g.C * g.To) return false;
    m.v = blockIdx.y;
    m.c = (int)(s / g.To);
    m.t = (int)(s - (int64_t)m.c * g.To);
    m.f0 = 0; m.F = g.F;
    if (g.vids) { const VidDesc vd = g.vids[m.v]; m.f0 = vd.f0; m.F = vd.F; }
    return true;
}

__device__ __forceinline__ int merge_count(const MergeSet &s, const MergeArgs &g, const MergeSlot &m)
{
    const int n = s.ntracks[(int64_t)m.v * g.C + m.c];
    return n < 0 ? 0 : (n > s.T ? s.T : n);
}

// first element of slot (c, t) of a [C,T,F_v] block with T slots per class
__device__ __forceinline__ int64_t merge_elem(const MergeArgs &g, const MergeSlot &m, int T, int t)
{
    return (int64_t)g.C * T * m.f0 + ((int64_t)m.c * T + t) * m.F;
}

// slot (set s, element se) -> output element oe: rows, tboxes, every series and the anchor, bit for bit
__device__ __forceinline__ void merge_copy_slot(const MergeArgs &g, const MergeSet &s, int64_t se, int64_t sslot, int64_t oe,
                                                int64_t oslot, int F, int lane)
{
    wave_copy_words(reinterpret_cast<uint32_t *>(g.otracks + oe * 5), reinterpret_cast<const uint32_t *>(s.tracks + se * 5),
                    (int64_t)F * 5, lane);
    if (g.otboxes)
        wave_copy_words(reinterpret_cast<uint32_t *>(g.otboxes + oe * 4), reinterpret_cast<const uint32_t *>(s.tboxes + se * 4),
                        (int64_t)F * 4, lane);
#pragma unroll
    for (int q = 0; q < kMergeMaxSeries; ++q)
        if (q < g.nser)
            wave_copy_words(reinterpret_cast<uint32_t *>(g.oseries + q * g.oN + oe),
                            reinterpret_cast<const uint32_t *>(s.series[q] + se), (int64_t)F * 2, lane);
    if (lane < 3) g.oanchors[oslot * 3 + lane] = s.anchors[sslot * 3 + lane];
}

__global__ __launch_bounds__(kMergeLT) void merge_combine_kernel(const MergeArgs g)
{
    MergeSlot m;
    if (!merge_slot(g, m)) return;
    const int lane = threadIdx.x & 63;
    const int nta = merge_count(g.a, g, m), ntb = merge_count(g.b, g, m);
    const int64_t oe = merge_elem(g, m, g.To, m.t);
    const int64_t oslot = ((int64_t)m.v * g.C + m.c) * g.To + m.t;
    if (m.t == 0 && lane == 0) g.ontracks[(int64_t)m.v * g.C + m.c] = nta + ntb;
    if (m.t < nta) {
        merge_copy_slot(g, g.a, merge_elem(g, m, g.a.T, m.t), ((int64_t)m.v * g.C + m.c) * g.a.T + m.t, oe, oslot, m.F, lane);
    } else if (m.t < nta + ntb) {
        const int u = m.t - nta;
        merge_copy_slot(g, g.b, merge_elem(g, m, g.b.T, u), ((int64_t)m.v * g.C + m.c) * g.b.T + u, oe, oslot, m.F, lane);
    } else {
        const uint32_t qnan = 0x7FC00000u;
        wave_fill_words(reinterpret_cast<uint32_t *>(g.otracks + oe * 5), (int64_t)m.F * 5, qnan, qnan, lane);
        if (g.otboxes) wave_fill_words(reinterpret_cast<uint32_t *>(g.otboxes + oe * 4), (int64_t)m.F * 4, qnan, qnan, lane);
#pragma unroll
        for (int q = 0; q < kMergeMaxSeries; ++q)
            if (q < g.nser)
                wave_fill_words(reinterpret_cast<uint32_t *>(g.oseries + q * g.oN + oe), (int64_t)m.F * 2, 0u, 0x7FF80000u, lane);
        if (lane < 3) g.oanchors[oslot * 3 + lane] = 0.0f;
    }
}

__global__ __launch_bounds__(kMergeLT) void merge_max_kernel(const MergeArgs g)
{
    MergeSlot m;
    if (!merge_slot(g, m)) return;          // (To == a.T)
    const int lane = threadIdx.x & 63;
    const int F = m.F;
    const int nta = merge_count(g.a, g, m), ntb = merge_count(g.b, g, m);
    const int64_t ae = merge_elem(g, m, g.a.T, m.t);
    const int64_t aslot = ((int64_t)m.v * g.C + m.c) * g.a.T + m.t;
    uint8_t *fb = g.from_b + ae;
    if (m.t == 0 && lane == 0) g.ontracks[(int64_t)m.v * g.C + m.c] = nta;
    const float *ta = g.a.tracks + ae * 5;
    int cnt = 0;                            // boxes of ordinal < cnt may take b's values
    int64_t be = 0;
    if (m.t < (nta < ntb ? nta : ntb)) {    // a paired slot (wave-uniform)
        be = merge_elem(g, m, g.b.T, m.t);
        const float *tb = g.b.tracks + be * 5;
        int ca = 0, cb = 0, k0 = 0x7FFFFFFF;
        for (int base = 0; base < F; base += 64) {
            const int f = base + lane;
            bool ea = false, eb = false;
            if (f < F) {
                const float x = ta[(int64_t)f * 5], y = tb[(int64_t)f * 5];
                ea = !(x != x); eb = !(y != y);
            }
            const unsigned long long ma = __ballot(ea), mb = __ballot(eb), x = ma ^ mb;
            if (x && k0 == 0x7FFFFFFF) k0 = ca + __popcll(ma & ((x & (0ull - x)) - 1ull));
            ca += __popcll(ma); cb += __popcll(mb);
        }
        cnt = ca < cb ? ca : cb;
        if (cnt >= 1) {
            const float fa = g.a.anchors[aslot * 3], fbn = g.b.anchors[(((int64_t)m.v * g.C + m.c) * g.b.T + m.t) * 3];
            const bool bad = k0 < cnt || !(truncf(fa) == truncf(fbn));
            if (bad) {
                if (lane == 0) atomicOr(g.status, kStBadMerge);
                cnt = 0;
            }
        }
    }
    if (cnt == 0) {                         // unpaired, nothing to pair or a latched violation: a copy of a
        merge_copy_slot(g, g.a, ae, aslot, ae, aslot, F, lane);
        for (int f = lane; f < F; f += 64) fb[f] = 0;
        return;
    }
    // Sweep 2.  The verdict of a chunk's 64 frames is a ballot; the chunk's rows (and tboxes) are then moved as ONE run of
    // words, lane w of a step taking word w from the side its frame w / 5 (w / 4) chose: coalesced dword loads and stores.
    const uint32_t *wa = reinterpret_cast<const uint32_t *>(ta), *wb = reinterpret_cast<const uint32_t *>(g.b.tracks + be * 5);
    uint32_t *wo = reinterpret_cast<uint32_t *>(g.otracks + ae * 5);
    int oa = 0;
    for (int base = 0; base < F; base += 64) {
        const int f = base + lane, nf = F - base < 64 ? F - base : 64;
        float r0 = __uint_as_float(0x7FC00000u);
        if (f < F) r0 = ta[(int64_t)f * 5];
        const bool ea = !(r0 != r0);
        const unsigned long long ma = __ballot(ea);
        bool take = false;
        if (ea && oa + __popcll(ma & ((1ull << lane) - 1ull)) < cnt) take = g.b.series[0][be + f] > g.a.series[0][ae + f];
        const unsigned long long tm = __ballot(take);
        {
            const int64_t o = (int64_t)base * 5;
            uint32_t v[5];
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                const int w = j * 64 + lane;
                v[j] = w < nf * 5 ? (((tm >> (w / 5)) & 1ull) ? wb : wa)[o + w] : 0u;
            }
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                const int w = j * 64 + lane;
                if (w < nf * 5) wo[o + w] = v[j];
            }
        }
        if (g.otboxes) {
            const uint32_t *xa = reinterpret_cast<const uint32_t *>(g.a.tboxes + (ae + base) * 4);
            const uint32_t *xb = reinterpret_cast<const uint32_t *>(g.b.tboxes + (be + base) * 4);
            uint32_t *xo = reinterpret_cast<uint32_t *>(g.otboxes + (ae + base) * 4);
            uint32_t v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int w = j * 64 + lane;
                v[j] = w < nf * 4 ? (((tm >> (w >> 2)) & 1ull) ? xb : xa)[w] : 0u;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int w = j * 64 + lane;
                if (w < nf * 4) xo[w] = v[j];
            }
        }
        if (f < F) {
#pragma unroll
            for (int q = 0; q < kMergeMaxSeries; ++q)
                if (q < g.nser) g.oseries[q * g.oN + ae + f] = take ? g.b.series[q][be + f] : g.a.series[q][ae + f];
            fb[f] = take ? 1 : 0;
        }
        oa += __popcll(ma);
    }
    if (lane < 3) g.oanchors[aslot * 3 + lane] = g.a.anchors[aslot * 3 + lane];
}

}  // namespace vdet
