// Per-frame NMS of tubelet boxes together with still-image detections: nms (utils/nms.pyx:17-68) of every (class, frame)
// list the pipeline emits -- what apply_vid_nms (vdet/video_det.py:51-61) does to a detection proto through vid_nms
// (utils/nms.pyx:71-125), whose frame test makes it one nms per frame.  Semantics in full: include/vdet_hip.h (vdet_nms_tracks).
//
// A LIST is the candidate rows of one (class c, frame f) in this order:
//   still-image rows  k < min(keep_cnt[f,c], top_still):  b = keep_idx[f,c,k], (boxes[f,b], scores[f,b,c])
//   tubelet rows      t < ntracks[c] with tracks[c,t,f,0] not NaN:  (tboxes[c,t,f] or tracks[c,t,f,0:4], (float)score[c,t,f])
// A row whose f32 score is NaN is absent.  Row INDEX j = k for a still-image row, ns + t for a tubelet row (ns = the list's
// still-image rows): absent rows leave holes, which changes no comparison of two indices.
//
// ONE launch, one WAVE per list, 1 / 2 / 4 waves per workgroup (the host picks the most that keeps the workgroup's LDS below
// 64 KiB), grid (ceil(C*Fmax / waves), V).  List s of a video is (c, f) = (s / F, s % F): the waves of a workgroup hold
// ADJACENT FRAMES of one class, so the 20-byte tubelet rows tracks[c,t,f..f+3] they gather, and the rank rows [c,r,f..f+3]
// they write, are one 80-byte run -- the lines a wave pulls in are the ones its neighbours need.  A lane's own loads are
// scalar dwords (a 20-byte row is 4-byte aligned, no more) and one dwordx4 for a still-image box or a tboxes row.
//
// Per wave, LDS: box [n] float4 and a 64-bit COMPOSITE [n], n = top_still + T of THE CALL (24 bytes per candidate; the typical
// list of 120 costs 2.9 KiB, the limit of 1024 costs 24 KiB and halves the waves per workgroup, nothing else).
//   composite = score_key(s) << 32 | j  while the row is alive (score_key > 0 for every non-NaN float),
//             = rank + 1                once it is kept (high word 0),
//             = 0                       absent or suppressed.
// Entry j is read and written by lane j & 63 alone; only the boxes are read across lanes (written once, one fence).
// SELECTION instead of a sort: the wave maximum of the alive composites is the next row of the reference's order (descending
// score, -0.0 == +0.0, equal scores by descending index) that is not suppressed -- it is kept, tested with pair_pred against
// every alive row (those are exactly the later, not yet suppressed rows: the pairs utils/nms.pyx:53-66 evaluates, so the
// zero-union flag of an evaluated pair is the reference's ZeroDivisionError), and the same sweep carries the maximum of the
// rows that stay alive, which is the next kept row.  Cost: kept x ceil(n / 64) pair tests per lane and six 64-bit shuffles
// per kept row.  No sort, no atomics in LDS, no scratch of the context.
// OUTPUT sweep: lane j & 63 reads the source of every kept row again (the lines are in cache) and writes rank row r of frame
// f: tracks [C,R,F,5], score [C,R,F] f64 (the source's own score, unrounded), src [C,R,F]; the ranks behind the count are
// filled with NaN / INT32_MIN.  cnt [C,F] = rows kept; ntracks [V,C] = max over the frames of min(cnt, R), by atomicMax on an
// integer the host zeroed.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nms_kernels.hpp"       // score_key, box_area, pair_pred, kStCap, kStDivZero
#include "batch_kernels.hpp"     // VidDesc

namespace vdet {

constexpr int kStBadKeep = 512;      // vdet_nms_tracks: a keep_cnt outside 0..cap or a read keep_idx outside 0..B-1
constexpr int kTnMaxList = 1024;     // top_still + T, and R: the evaluator's tracks-per-(frame, class) limit
constexpr int kTnBytesPerCand = 24;  // float4 box + 64-bit composite
constexpr int kTnSrcPad = INT32_MIN;

struct TrackNmsArgs {
    // tubelets (batch: video v at element C*T*f0)
    const float *tracks;        // [C,T,F,5]; null when T == 0
    const int32_t *ntracks;     // [V,C]
    const void *score;          // [C,T,F] f32 or f64
    const float4 *tboxes;       // [C,T,F] or null
    // still-image source, frame-major over all videos; null without it (top_still == 0)
    const float4 *boxes;        // [Ftot,B]
    const float *scores;        // [Ftot,B,C]
    const int32_t *keep_idx;    // [Ftot,C,cap]
    const int32_t *keep_cnt;    // [Ftot,C]
    const VidDesc *vids;        // null: one video of F frames
    int F, Ftot, C, T, B, cap, top_still, R, nmax, score_f64;
    float t32;
    float *otracks;             // [C,R,F,5]  (batch: video v at element C*R*f0)
    double *oscore;             // [C,R,F]
    int32_t *osrc;              // [C,R,F]
    int32_t *ocnt;              // [C,Ftot]
    int32_t *ontracks;          // [V,C], zeroed by the host
    int *status;
};

struct TnList { int c, f, F, ns, n; int64_t fg, tbase, obase; };

struct TnRow { float4 box; float s32; double s64; int32_t src; };

__device__ __forceinline__ unsigned long long tn_wave_max(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const unsigned long long x = __shfl_xor(v, o, 64);
        v = x > v ? x : v;
    }
    return v;
}

// candidate j of the list: false where the row is absent.  bad: the row's keep_idx is out of range (the row is skipped)
__device__ __forceinline__ bool tn_load_row(const TrackNmsArgs &g, const TnList &m, int j, TnRow &r, bool &bad)
{
    if (j < m.ns) {
        const int b = g.keep_idx[(m.fg * g.C + m.c) * g.cap + j];
        if (b < 0 || b >= g.B) { bad = true; return false; }
        const int64_t e = m.fg * g.B + b;
        r.box = g.boxes[e];
        r.s32 = g.scores[e * g.C + m.c];
        r.s64 = (double)r.s32;
        r.src = b;
    } else {
        const int t = j - m.ns;
        const int64_t e = m.tbase + (int64_t)t * m.F;
        const float *row = g.tracks + e * 5;
        const float x1 = row[0];
        if (x1 != x1) return false;
        r.box = g.tboxes ? g.tboxes[e] : make_float4(x1, row[1], row[2], row[3]);
        if (g.score_f64) { r.s64 = static_cast<const double *>(g.score)[e]; r.s32 = (float)r.s64; }
        else { r.s32 = static_cast<const float *>(g.score)[e]; r.s64 = (double)r.s32; }
        r.src = -(t + 1);
    }
    return !(r.s32 != r.s32);
}

// ---- the pieces every rule on these lists calls (softnms_kernels.hpp, votenms_kernels.hpp) ----

// OPEN: the list of wave w of the nw in this workgroup.  false: the wave is past the C * F_v lists of its video.  bad is set where
// keep_cnt is outside 0..cap (the list then has no still-image rows)
__device__ __forceinline__ bool tn_open(const TrackNmsArgs &g, int nw, int w, TnList &m, bool &bad)
{
    const int v = blockIdx.y;
    int64_t f0 = 0;
    m.F = g.F;
    if (g.vids) { const VidDesc vd = g.vids[v]; f0 = vd.f0; m.F = vd.F; }
    const int64_t s = (int64_t)blockIdx.x * nw + w;
    if (s >= (int64_t)g.C * m.F) return false;
    m.c = (int)(s / m.F);
    m.f = (int)(s - (int64_t)m.c * m.F);
    m.fg = f0 + m.f;
    m.tbase = (int64_t)g.C * g.T * f0 + (int64_t)m.c * g.T * m.F + m.f;
    m.obase = (int64_t)g.C * g.R * f0 + (int64_t)m.c * g.R * m.F + m.f;
    m.ns = 0;
    if (g.top_still > 0) {
        const int kc = g.keep_cnt[m.fg * g.C + m.c];
        if (kc < 0 || kc > g.cap) bad = true;
        else m.ns = kc < g.top_still ? kc : g.top_still;
    }
    int nt = 0;
    if (g.T > 0) {
        nt = g.ntracks[(int64_t)v * g.C + m.c];
        nt = nt < 0 ? 0 : (nt > g.T ? g.T : nt);
    }
    m.n = m.ns + nt;                                     // (<= top_still + T = nmax)
    return true;
}

// LDS carve: [nw][nmax] of each plane -- boxes (16 B per candidate), composites (8 B), then the 4-byte planes k = 0, 1, ...
struct TnLds {
    unsigned char *smem;
    size_t all, mine;                                    // nw * nmax, w * nmax
    __device__ __forceinline__ TnLds(unsigned char *base, int nw, int w, int nmax) : smem(base), all((size_t)nw * nmax), mine((size_t)w * nmax) {}
    __device__ __forceinline__ float4 *box() const { return reinterpret_cast<float4 *>(smem) + mine; }
    __device__ __forceinline__ unsigned long long *comp() const { return reinterpret_cast<unsigned long long *>(smem + all * 16) + mine; }
    template <typename T> __device__ __forceinline__ T *plane(int k) const
    {
        static_assert(sizeof(T) == 4, "a 4-byte plane");
        return reinterpret_cast<T *>(smem + all * (24 + 4 * k)) + mine;
    }
};

// HARD SELECTION (the header's SELECTION paragraph): best = the lane's maximum of the gathered composites.  on_keep(rank, j)
// runs in the lane that marks row j kept.  Returns the rows kept; zero is set by an evaluated zero-union pair.
template <typename OnKeep>
__device__ __forceinline__ int tn_select(const TrackNmsArgs &g, const TnList &m, int lane, const float4 *sbox,
                                         unsigned long long *scomp, unsigned long long best, bool &zero, OnKeep on_keep)
{
    int kept = 0;
    for (;;) {
        const unsigned long long top = tn_wave_max(best);
        const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(top >> 32));
        if (hi == 0u) break;
        const int i = __builtin_amdgcn_readfirstlane((int)(unsigned)top);
        const float4 bi = sbox[i];
        const float ai = box_area(bi);
        best = 0ull;
        for (int j = lane; j < m.n; j += 64) {
            const unsigned long long k = scomp[j];
            if ((k >> 32) == 0ull) continue;
            if (j == i) { scomp[j] = (unsigned long long)(kept + 1); on_keep(kept, j); continue; }
            const float4 bj = sbox[j];
            const uint32_t p = pair_pred(bi, ai, bj, box_area(bj), g.t32);
            if (p & 2u) zero = true;
            if (p & 1u) scomp[j] = 0ull;
            else best = k > best ? k : best;
        }
        ++kept;
    }
    return kept;
}

// rank row e of the common outputs
__device__ __forceinline__ void tn_store_row(const TrackNmsArgs &g, int64_t e, float4 box, float s32, double s64, int32_t src)
{
    float *o = g.otracks + e * 5;
    o[0] = box.x; o[1] = box.y; o[2] = box.z; o[3] = box.w; o[4] = s32;
    g.oscore[e] = s64;
    g.osrc[e] = src;
}

// the fill of a rank row behind the count
__device__ __forceinline__ void tn_store_pad(const TrackNmsArgs &g, int64_t e)
{
    const float qnan = __uint_as_float(0x7FC00000u);
    float *o = g.otracks + e * 5;
    o[0] = qnan; o[1] = qnan; o[2] = qnan; o[3] = qnan; o[4] = qnan;
    g.oscore[e] = __longlong_as_double(0x7FF8000000000000ll);
    g.osrc[e] = kTnSrcPad;
}

// CLOSE: cnt of the list, ntracks of its (video, class), the status bits of the wave.  The two flags come by reference: copied
// into parameters they stay SGPR lane masks through every loop, which took softnms_kernel to 105 SGPRs (7 waves per SIMD, not 8)
__device__ __forceinline__ void tn_close(const TrackNmsArgs &g, const TnList &m, int lane, int count, const bool &bad, const bool &zero)
{
    const unsigned long long anybad = __ballot(bad), anyzero = __ballot(zero);
    if (lane == 0) {
        g.ocnt[(int64_t)m.c * g.Ftot + m.fg] = count;
        const int live = count < g.R ? count : g.R;
        if (live > 0) atomicMax(g.ontracks + (int64_t)blockIdx.y * g.C + m.c, live);
        const int st = (anybad ? kStBadKeep : 0) | (anyzero ? kStDivZero : 0) | (count > g.R ? kStCap : 0);
        if (st) atomicOr(g.status, st);
    }
}

__global__ __launch_bounds__(256) void tracknms_kernel(const TrackNmsArgs g)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char tn_smem[];
    const int lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    TnList m;
    bool badkeep = false;
    if (!tn_open(g, nw, w, m, badkeep)) return;
    const TnLds lds(tn_smem, nw, w, g.nmax);
    float4 *sbox = lds.box();
    unsigned long long *scomp = lds.comp();

    // gather
    unsigned long long best = 0ull;
    for (int j = lane; j < m.n; j += 64) {
        TnRow r;
        unsigned long long k = 0ull;
        if (tn_load_row(g, m, j, r, badkeep)) {
            sbox[j] = r.box;
            k = ((unsigned long long)score_key(r.s32) << 32) | (unsigned)j;
        }
        scomp[j] = k;
        best = k > best ? k : best;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();

    bool zero = false;
    const int kept = tn_select(g, m, lane, sbox, scomp, best, zero, [](int, int) {});

    // output: the kept rows at their ranks, the fill behind the count
    for (int j = lane; j < m.n; j += 64) {
        const unsigned long long k = scomp[j];
        if ((k >> 32) != 0ull || k == 0ull) continue;
        const int r = (int)k - 1;
        if (r >= g.R) continue;
        TnRow row;
        bool dummy = false;
        tn_load_row(g, m, j, row, dummy);
        tn_store_row(g, m.obase + (int64_t)r * m.F, row.box, row.s32, row.s64, row.src);
    }
    for (int r = (kept < g.R ? kept : g.R) + lane; r < g.R; r += 64) tn_store_pad(g, m.obase + (int64_t)r * m.F);
    tn_close(g, m, lane, kept, badkeep, zero);
}

}  // namespace vdet

