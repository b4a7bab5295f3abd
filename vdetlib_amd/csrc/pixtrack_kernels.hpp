// Device pixel tracker: tubelets that follow the PIXELS of an anchor box through the frames (the role of the reference's
// fcn_tracker, vdet/track.py:52-106; not its arithmetic: that is external MATLAB), in the [C,T,F,5] layout of the anchor route.
// The rule is tests/pixtrack_spec.py, integers on uint8 pixels; the device matches it bit for bit.
//
//   luma      L = (29*c0 + 150*c1 + 77*c2 + 128) >> 8 on the stored channel order
//   grid      box (x1,y1,x2,y2) 0-based, w = x2-x1+1, side S: cell k samples column clamp(x1 + floor((2k+1)*w / 2S), 0, W-1),
//             rows likewise (point sampling, edge replication)
//   template  the grid k = 0..S-1 of the (truncated, minus one) anchor box on the anchor frame, fixed for both directions
//   step      f -> g = f +- step: the region is the grid k = -R..S+R-1 of the current box on frame g; every (dy,dx) in
//             [-R,R]^2 gets SAD = sum |Tm[i,j] - Rg[i+R+dy, j+R+dx]|; the smallest key (SAD, dy^2+dx^2, dy, dx) wins;
//             conf = 1.0f - float(SAD) / float(255*S*S); conf < (float)min_conf ends the chain; the box moves by
//             floor((2*dx*w + S) / 2S), floor((2*dy*h + S) / 2S); a box wholly outside the image ends the chain; else the row
//             (x1+1, y1+1, x2+1, y2+1, conf) is written
//   bad data  an anchor frame outside 0..F; on a live slot a box that is not finite, has |coordinate| > 2^20, w < 1 or h < 1
//             after truncation, or lies wholly outside the image: kStBadPixAnchor, the slot is written as an empty one
//
// Shape: anchor_link_kernel's.  ONE launch, grid (C*T, 2), a workgroup per chain (slot x direction); the forward block
// writes the anchor row, the anchors entry, a dead slot's NaN rows and -- slot 0 of a class -- ntracks; every output element
// is written exactly once by this launch (a chain's own rows by thread 0, the rows it does not reach -- beyond its end and on
// the frames step > 1 skips -- by the whole block afterwards).  A chain is a dependent walk; the parallelism is across the
// chains and inside a step:
//   1. the first 2*(S+2R) threads make the step's column / row tables (one floor division each);
//   2. the block gathers the (S+2R)^2 region, luma from the three bytes in flight, four pixels to a dword of LDS;
//   3. the (2R+1)^2 candidates are spread over the lanes; a candidate is S*S/4 v_sad_u8 on dwords that v_alignbyte_b32 cuts
//      from two neighbouring region dwords (the template dword is the same address in every lane: an LDS broadcast);
//   4. the key packed in 64 bits (SAD | dy^2+dx^2 | dy+R | dx+R) is min-reduced by wave shuffles, then over the waves through
//      an LDS slot per wave, double-buffered by step parity.  Keys are unique, so the order of the reduction cannot matter;
//      every lane derives the new box from the winning key.
// LDS: region 96 x 25 dwords (one spare dword per row for the pair read at shift 0) + template 64 x 16 dwords + tables:
// 14.2 KiB, static.  Nothing of the context's cached graph, lists, index or link memo is read or written.
//
// The chain is pix_chain, a device function: track_pixels_kernel runs it from a slot table, track_pixel_chain_kernel -- the
// tracker of the greedy loop vdet_track_volume_pixels (the rule's greedy loop) -- from the anchor the pick left in TrackState.
//
// Scale search (the rule's ``scales``; track_pixels_scaled_kernel, track_pixel_chain_scaled_kernel): pix_chain<true>.
// Per step, for every level l in -ns..ns the box is grown about its centre by ex = sgn(l) * floor((|l|*p*w + 100) / 200) columns
// and ey rows a side (l != 0 is skipped when a side falls below 1 or exceeds 2^21: block-uniform); each admissible level gets
// its own tables, gather and SAD pass over the SAME S x S template, a lane keeps its smallest key across the levels in
// registers, and the ONE reduction of the step follows the last level.  The key is (SAD + |l|*q | |l| | dy^2+dx^2 | dy+R | dx+R
// | l+3): the raw SAD of the winner is key_hi - |l|*q.  The box state (x1, y1, w, h) stays scalar; the winner's level box,
// moved, is the new box.  pix_chain<false> is the fixed-scale chain, the code it was before the template.
//
// Box sampling (the rule's ``sampling='box'``; track_pixels_box_kernel, track_pixel_chain_box_kernel): pix_chain<true, true>.
// A cell's value is the rounded mean of its pixels instead of one pixel, read from a summed-area table of the luma:
//   integral  I[f, y, x] = sum of L[f, r, c] over r < y, c < x, uint32 [F, H+1, W+1]; H*W <= 2^24, so 255 * 2^24 fits
//   edges     per axis: a = o + floor(k*e / S), b = o + floor((k+1)*e / S), a' = clamp(a, 0, N-1), b' = min(max(b, a'+1), N)
//   value     tot = I[rb', cb'] - I[ra', cb'] - I[rb', ca'] + I[ra', ca'], area = (rb'-ra') * (cb'-ca'), (tot + (area >> 1)) / area
// The step's tables hold a' and b' per cell and axis (two floor divisions a thread), the gather reads four integral entries
// per cell and divides (an exact u32 division); the template is gathered the same way from the anchor frame's integral.  The
// SAD pass, the reduction and the box state are the point chain's.  PixTrackArgs::images carries the integral in this mode; the
// chain always runs the level loop (scales = 0: one trip, the fixed-scale chain's winner).  LDS: two more tables, 15.0 KiB.
//
// Template update with an anchor guard (the rule's ``update``, tests/pixtrack_adapt_spec.py; track_pixels_adaptive[_box]_kernel,
// track_pixel_chain_adaptive[_box]_kernel): pix_chain<true, BOX, true>.  Per chain (slot AND direction) the state is A[S,S] in 8.8
// fixed point, A = Tm0 << 8 at the start; a step matches against Tm = (A + 128) >> 8, which is what stm holds.  After a step the
// chain keeps, with P the S x S window that won (cells dx.., dy.. of the winner's level box on frame g, before the move):
//   guard     SAD0 = sum |Tm0 - P|, c0 = 1.0f - float(SAD0) / float(255*S*S)
//   accept    a > 0 and conf >= (float)update_conf and c0 >= (float)drift_conf
//   update    A = ((256 - a) * A + a * (P << 8) + 128) >> 8 per cell (<= 256 * 65280 + 128: 32 bits), Tm follows
// The state costs no LDS: thread t owns the template dwords t, t + 256, ... (at most 4: 16 cells at S = 64) and keeps their Tm0
// bytes (4 registers) and their A as 16-bit pairs (8 registers); after an accepted step it rewrites only its own dwords of stm.
// P is read from the region still in sreg when the winner's level was the last one gathered, else the S x S window is gathered
// again (the tables take one first cell per axis for this).  SAD0 is one v_sad_u8 per owned dword, wave shuffles, a slot per
// wave in LDS (16 bytes) and one barrier; the decision is block-uniform.  The barriers that order the hazards -- the SAD pass's
// reads of stm before the update's writes, those writes before the next SAD pass, sreg and the tables under the re-gather --
// are named where the code stands, in pix_chain.
//
// The integral is made by two launches (vdet_luma_integral), luma in flight, no luma plane in memory:
//   luma_integral_rows_kernel  a wave per image row: 64 pixels a trip, a wave scan, the carry of the trips so far in a register;
//                              writes I[f, y+1, 1..W] = the row's prefix sums and I[f, y+1, 0] = 0
//   luma_integral_cols_kernel  a thread per column of a frame, rows top to bottom (a wave reads and writes 256 contiguous
//                              bytes of a row), eight rows' loads in flight; writes row 0 = 0 and the sums in place
// Sums are exact, so the order of the additions is free.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "track_kernels.hpp"

namespace vdet {

constexpr int kStBadPixAnchor = 4096;    // vdet_track_pixels: an anchor frame outside 0..F or an anchor box that cannot be tracked
constexpr int kPixLT = 256;              // threads per chain
constexpr int kPixWaves = kPixLT / 64;
constexpr int kPixMaxS = 64, kPixMaxR = 16;
constexpr int kPixMaxP = kPixMaxS + 2 * kPixMaxR;       // region side
constexpr int kPixMaxPitch = kPixMaxP / 4 + 1;          // region row pitch in dwords (one spare: see the pair read)
constexpr int kPixCoordMax = 1 << 20;
constexpr int kPixSideMax = 1 << 21;     // scale search: a level whose box is wider or higher is skipped (products stay in int32)
constexpr int64_t kPixBoxMaxArea = 1 << 24;       // box sampling: H * W of a frame (255 * 2^24 is the largest integral entry)
constexpr int kPixMaxScales = 3, kPixMaxScaleStep = 25, kPixMaxScalePenalty = 65535;

struct PixTrackArgs {
    const uint8_t *images;      // [F,H,W,3]; box sampling: the integral, uint32 [F,H+1,W+1]
    int F, H, W, C, T;
    const int32_t *aframes;     // [C,T] 1-based, 0: empty slot
    const float *aboxes;        // [C,T,4]
    const float *ascores;       // [C,T] or null
    int S, R;
    float min_conf;
    int reach, step;
    float *tracks;              // [C,T,F,5]
    float *anchors;             // [C,T,3]
    int32_t *ntracks;           // [C]
    int *status;
};

// the scale search of pix_chain<true>: ns levels each side (0 .. 3), p percent per level (1 .. 25), q SAD units per level
struct PixScaleArgs {
    int ns, p, q;
};

// the template update of pix_chain<true, BOX, true>: a = the weight of the new patch in 1/256 (0 .. 256; 0: never), the update
// is accepted at conf >= update_conf and c0 >= drift_conf (f32 compares)
struct PixAdaptArgs {
    int a;
    float update_conf, drift_conf;
};
constexpr int kPixOwn = kPixMaxS * (kPixMaxS / 4) / kPixLT;     // template dwords a thread owns (tid, tid + 256, ...): 4, 16 cells

__device__ __forceinline__ int pix_floordiv(int a, int b)      // b > 0
{
    int q = a / b;
    if (a - q * b < 0) --q;
    return q;
}

// the columns (rows) level l != 0 adds on each side of a box e wide (high): sgn(l) * floor((|l|*p*e + 100) / 200).
// e <= 2^21 + 1, |l|*p <= 75: the product stays below 2^28
__device__ __forceinline__ int pix_level_margin(int l, int p, int e)
{
    const int al = l < 0 ? -l : l;
    const int m = (al * p * e + 100) / 200;
    return l < 0 ? -m : m;
}

__device__ __forceinline__ bool pix_outside(int x1, int y1, int x2, int y2, int H, int W)
{
    return x2 < 0 || y2 < 0 || x1 > W - 1 || y1 > H - 1;
}

// the box a chain starts from: -1: cannot be tracked, 1: b = the 0-based integer box (truncated toward zero, minus one)
__device__ __forceinline__ int pix_box_state(const float *p, int H, int W, int4 &b)
{
    const float lim = (float)kPixCoordMax;
    const float v0 = p[0], v1 = p[1], v2 = p[2], v3 = p[3];
    // (a NaN fails every comparison, an infinity the bound)
    if (!(fabsf(v0) <= lim && fabsf(v1) <= lim && fabsf(v2) <= lim && fabsf(v3) <= lim)) return -1;
    b = make_int4((int)v0 - 1, (int)v1 - 1, (int)v2 - 1, (int)v3 - 1);
    if (b.z - b.x + 1 < 1 || b.w - b.y + 1 < 1 || pix_outside(b.x, b.y, b.z, b.w, H, W)) return -1;
    return 1;
}

// 0: empty slot, -1: bad data, 1: live and b = the 0-based integer box
__device__ __forceinline__ int pix_anchor_state(const PixTrackArgs &a, int64_t slot, int4 &b)
{
    const int fr = a.aframes[slot];
    if (fr < 0 || fr > a.F) return -1;
    if (fr == 0) return 0;
    return pix_box_state(a.aboxes + slot * 4, a.H, a.W, b);
}

__device__ __forceinline__ uint32_t pix_luma(const uint8_t *p)
{
    return (29u * p[0] + 150u * p[1] + 77u * p[2] + 128u) >> 8;
}

// the tables of the grid k = k0x .. k0x+n-1 (columns), k0y .. k0y+n-1 (rows) of the box: tcol[i] = 3 * column, trow[i] = row.
// n <= kPixMaxP, 2n <= kPixLT.
__device__ __forceinline__ void pix_tables(int *tcol, int *trow, int x1, int y1, int w, int h, int S, int k0x, int k0y, int n, int H,
                                           int W)
{
    const int tid = threadIdx.x;
    if (tid < 2 * n) {
        const bool isrow = tid >= n;
        const int i = isrow ? tid - n : tid;
        const int o = isrow ? y1 : x1, e = isrow ? h : w, lim = isrow ? H : W, k0 = isrow ? k0y : k0x;
        int v = o + pix_floordiv((2 * (k0 + i) + 1) * e, 2 * S);
        v = v < 0 ? 0 : (v > lim - 1 ? lim - 1 : v);
        if (isrow) trow[i] = v;
        else tcol[i] = 3 * v;
    }
}

// n x n lumas of one frame into dst (row pitch `pitch` dwords, all of them written; bytes beyond n are 0)
__device__ __forceinline__ void pix_gather(uint32_t *dst, int pitch, const int *tcol, const int *trow, int n,
                                           const uint8_t *frame, int W)
{
    const int total = n * pitch;
    for (int d = threadIdx.x; d < total; d += kPixLT) {
        const int i = d / pitch, q = d - i * pitch;
        const uint8_t *rp = frame + (int64_t)trow[i] * W * 3;
        uint32_t v = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int j = 4 * q + b;
            if (j < n) v |= pix_luma(rp + tcol[j]) << (8 * b);
        }
        dst[d] = v;
    }
}

// box sampling: the edges of the cells k = k0x .. k0x+n-1 (columns), k0y .. k0y+n-1 (rows) of the box, ca/cb[i] = a'/b' of the
// columns, ra/rb[i] of the rows.  |k| <= 80 and e <= 2^21 + 1: the products stay below 2^28.  n <= kPixMaxP, 2n <= kPixLT.
__device__ __forceinline__ void pix_tables_box(int *ca, int *cb, int *ra, int *rb, int x1, int y1, int w, int h, int S, int k0x, int k0y,
                                               int n, int H, int W)
{
    const int tid = threadIdx.x;
    if (tid < 2 * n) {
        const bool isrow = tid >= n;
        const int i = isrow ? tid - n : tid;
        const int o = isrow ? y1 : x1, e = isrow ? h : w, lim = isrow ? H : W, k0 = isrow ? k0y : k0x;
        int lo = o + pix_floordiv((k0 + i) * e, S), hi = o + pix_floordiv((k0 + i + 1) * e, S);
        lo = lo < 0 ? 0 : (lo > lim - 1 ? lim - 1 : lo);
        hi = hi < lo + 1 ? lo + 1 : hi;
        hi = hi > lim ? lim : hi;
        if (isrow) { ra[i] = lo; rb[i] = hi; }
        else { ca[i] = lo; cb[i] = hi; }
    }
}

// pix_gather from one frame's integral I (row pitch pw = W + 1): n x n rounded cell means.  Every index is inside the frame's
// table: 0 <= a' < b' <= N.  tot <= 255 * area and area <= 2^24: the sums stay in 32 bits
__device__ __forceinline__ void pix_gather_box(uint32_t *dst, int pitch, const int *ca, const int *cb, const int *ra, const int *rb,
                                               int n, const uint32_t *I, int pw)
{
    const int total = n * pitch;
    for (int d = threadIdx.x; d < total; d += kPixLT) {
        const int i = d / pitch, q = d - i * pitch;
        const int r0 = ra[i], r1 = rb[i];
        const uint32_t *p0 = I + (int64_t)r0 * pw, *p1 = I + (int64_t)r1 * pw;
        const uint32_t hgt = (uint32_t)(r1 - r0);
        uint32_t v = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int j = 4 * q + b;
            if (j < n) {
                const int c0 = ca[j], c1 = cb[j];
                const uint32_t tot = (p1[c1] - p0[c1]) - (p1[c0] - p0[c0]);
                const uint32_t area = hgt * (uint32_t)(c1 - c0);
                v |= ((tot + (area >> 1)) / area) << (8 * b);
            }
        }
        dst[d] = v;
    }
}

// every row of a slot without a tubelet
__device__ __forceinline__ void pix_no_rows(float *trk, int F)
{
    const float qnan = __uint_as_float(0x7FC00000u);
    for (int64_t i = threadIdx.x; i < (int64_t)F * 5; i += kPixLT) trk[i] = qnan;
}

// One half of a live slot's tubelet, by the whole block: the chain from frame af (0-based) and box ab in direction dir, into the
// slot's rows trk [F,5].  The forward half (dir > 0) also writes the anchor row.  Every row of the half is written exactly once:
// the chain's own by thread 0, those it does not reach -- beyond its end and on the frames step > 1 skips -- by the whole block
// afterwards.  Reads of a: images, F, H, W, S, R, min_conf, reach, step.  Block-uniform control flow.
// SCALED: the scale search over the levels -sc.ns .. sc.ns (see the top of this file); otherwise sc is not read.
// BOX: box sampling from the integral a.images carries (see the top of this file).
// ADAPT: the template update with the anchor guard (see the top of this file); otherwise ad is not read.
template <bool SCALED, bool BOX = false, bool ADAPT = false>
__device__ __forceinline__ void pix_chain(const PixTrackArgs &a, float *trk, const int af, const int4 ab, const int dir,
                                          const PixScaleArgs sc, const PixAdaptArgs ad = PixAdaptArgs{0, 0.0f, 0.0f})
{
    static_assert(SCALED || !ADAPT, "the adaptive chain always runs the level loop");
    __shared__ uint32_t ssad0[ADAPT ? kPixWaves : 1];           // (ADAPT) the guard's SAD, a slot per wave
    __shared__ uint32_t sreg[kPixMaxP * kPixMaxPitch];
    __shared__ uint32_t stm[kPixMaxS * (kPixMaxS / 4)];
    __shared__ int tcol[kPixMaxP], trow[kPixMaxP];
    __shared__ int tcolb[BOX ? kPixMaxP : 1], trowb[BOX ? kPixMaxP : 1];         // (BOX: tcol / trow hold a', these b')
    __shared__ unsigned long long skey[2][kPixWaves];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int F = a.F, H = a.H, W = a.W, S = a.S, R = a.R;
    const float qnan = __uint_as_float(0x7FC00000u);
    // the box state is the same in every lane: keep it in scalar registers
    int x1 = __builtin_amdgcn_readfirstlane(ab.x), y1 = __builtin_amdgcn_readfirstlane(ab.y);
    int w = __builtin_amdgcn_readfirstlane(ab.z - ab.x + 1), h = __builtin_amdgcn_readfirstlane(ab.w - ab.y + 1);     // (fixed unless SCALED)
    if (dir > 0 && tid == 0) {
        float *r = trk + (int64_t)af * 5;
        r[0] = (float)(x1 + 1); r[1] = (float)(y1 + 1); r[2] = (float)(x1 + w); r[3] = (float)(y1 + h); r[4] = 1.0f;
    }
    const int64_t frame_bytes = (int64_t)H * W * 3;
    const uint32_t *integ = reinterpret_cast<const uint32_t *>(a.images);       // (BOX)
    const int64_t frame_cells = (int64_t)(H + 1) * (W + 1);
    const int P = S + 2 * R, pitch = P / 4 + 1, tq = S / 4, side = 2 * R + 1, ncand = side * side;
    // the template
    if constexpr (BOX) {
        pix_tables_box(tcol, tcolb, trow, trowb, x1, y1, w, h, S, 0, 0, S, H, W);
        __syncthreads();
        pix_gather_box(stm, tq, tcol, tcolb, trow, trowb, S, integ + (int64_t)af * frame_cells, W + 1);
    } else {
        pix_tables(tcol, trow, x1, y1, w, h, S, 0, 0, S, H, W);
        __syncthreads();
        pix_gather(stm, tq, tcol, trow, S, a.images + (int64_t)af * frame_bytes, W);
    }
    __syncthreads();
    const float denom = (float)(255 * S * S);
    // (ADAPT) the chain's state, in the registers of the thread that owns the cells: thread t owns the template dwords
    // t, t + 256, ... (kPixOwn of them at S = 64; none beyond S*S/4), that is four cells a dword.  tm0: the anchor's template
    // Tm0, as gathered; acc: A in 8.8, cells 0|1 and 2|3 of a dword packed in 16-bit halves.  Every loop over them is fully
    // unrolled, so the arrays are registers.
    uint32_t tm0[ADAPT ? kPixOwn : 1], acc[ADAPT ? 2 * kPixOwn : 1];
    if constexpr (ADAPT) {
#pragma unroll
        for (int k = 0; k < kPixOwn; ++k) {
            const int d = tid + k * kPixLT;
            const uint32_t v = d < S * tq ? stm[d] : 0u;
            tm0[k] = v;
            acc[2 * k] = ((v & 0xFFu) << 8) | ((v & 0xFF00u) << 16);
            acc[2 * k + 1] = ((v >> 8) & 0xFF00u) | (v & 0xFF000000u);
        }
    }

    int n = 0;                   // steps taken so far (block-uniform)
    for (int s = 1; s <= a.reach; ++s) {
        const int64_t g64 = (int64_t)af + (int64_t)dir * s * a.step;
        if (g64 < 0 || g64 >= F) break;
        const int g = (int)g64, par = s & 1;
        unsigned long long key = ~0ull;          // the lane's smallest key, across the levels
        const int ns = SCALED ? sc.ns : 0;
        for (int l = -ns; l <= ns; ++l) {        // (block-uniform; one trip at level 0 unless SCALED)
            int lx1 = x1, ly1 = y1, lw = w, lh = h;
            if constexpr (SCALED) {
                if (l != 0) {
                    const int ex = pix_level_margin(l, sc.p, w), ey = pix_level_margin(l, sc.p, h);
                    lw = w + 2 * ex;
                    lh = h + 2 * ey;
                    if (lw < 1 || lh < 1 || lw > kPixSideMax || lh > kPixSideMax) continue;
                    lx1 = x1 - ex;
                    ly1 = y1 - ey;
                }
            }
            // (the readers of the tables and of the region are behind a barrier: the template's below, the step's last one.
            // Between two levels of a step no barrier is added: the tables are read by the gather only, which every thread has
            // left at the barrier behind it, and the barrier behind these tables stands between the previous level's SAD reads
            // of the region and this level's gather, which overwrites it)
            if constexpr (BOX) {
                pix_tables_box(tcol, tcolb, trow, trowb, lx1, ly1, lw, lh, S, -R, -R, P, H, W);
                __syncthreads();
                pix_gather_box(sreg, pitch, tcol, tcolb, trow, trowb, P, integ + (int64_t)g * frame_cells, W + 1);
            } else {
                pix_tables(tcol, trow, lx1, ly1, lw, lh, S, -R, -R, P, H, W);
                __syncthreads();
                pix_gather(sreg, pitch, tcol, trow, P, a.images + (int64_t)g * frame_bytes, W);
            }
            __syncthreads();
            for (int cand = tid; cand < ncand; cand += kPixLT) {
                const int cy = cand / side, cx = cand - cy * side;      // dy + R, dx + R
                const int sh = cx & 3;
                const uint32_t *rrow = sreg + cy * pitch + (cx >> 2);
                const uint32_t *tp = stm;
                uint32_t sad = 0;
                for (int i = 0; i < S; ++i) {
                    uint32_t lo = rrow[0];
                    for (int q = 0; q < tq; ++q) {
                        const uint32_t hi = rrow[q + 1];
                        sad = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(hi, lo, sh), tp[q], sad);
                        lo = hi;
                    }
                    rrow += pitch;
                    tp += tq;
                }
                const int dy = cy - R, dx = cx - R;
                unsigned long long k;
                if constexpr (SCALED) {
                    // SAD + |l|*q <= 255*64*64 + 3*65535; dy^2+dx^2 <= 512: 10 bits; cy, cx <= 32; l + 3 in 0 .. 6
                    const uint32_t al = (uint32_t)(l < 0 ? -l : l);
                    const uint32_t low = (al << 28) | ((uint32_t)(dy * dy + dx * dx) << 18) | ((uint32_t)cy << 11) | ((uint32_t)cx << 3) |
                                         (uint32_t)(l + kPixMaxScales);
                    k = ((unsigned long long)(sad + al * (uint32_t)sc.q) << 32) | (unsigned long long)low;
                } else {
                    k = ((unsigned long long)sad << 32) | ((unsigned long long)(dy * dy + dx * dx) << 16) |
                        ((unsigned long long)cy << 8) | (unsigned long long)cx;
                }
                key = k < key ? k : key;
            }
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            const unsigned long long k2 = __shfl_xor(key, d, 64);
            key = k2 < key ? k2 : key;
        }
        if (lane == 0) skey[par][wv] = key;
        __syncthreads();
        key = skey[par][0];
#pragma unroll
        for (int k = 1; k < kPixWaves; ++k) {
            const unsigned long long k2 = skey[par][k];
            key = k2 < key ? k2 : key;
        }
        uint32_t sad = (uint32_t)(key >> 32);
        int dy, dx;
        if constexpr (SCALED) {
            const uint32_t low = (uint32_t)key, al = low >> 28;
            sad -= al * (uint32_t)sc.q;          // the confidence is the raw SAD's
            dy = (int)((low >> 11) & 0x7F) - R;
            dx = (int)((low >> 3) & 0xFF) - R;
            const int l = __builtin_amdgcn_readfirstlane((int)(low & 7u) - kPixMaxScales);
            if (l != 0) {                        // the winner's level box is the box that moves
                const int ex = pix_level_margin(l, sc.p, w), ey = pix_level_margin(l, sc.p, h);
                x1 -= ex;
                y1 -= ey;
                w += 2 * ex;
                h += 2 * ey;
            }
        } else {
            dy = (int)((key >> 8) & 0xFF) - R;
            dx = (int)(key & 0xFF) - R;
        }
        const float conf = 1.0f - (float)sad / denom;
        if (conf < a.min_conf) break;
        x1 = __builtin_amdgcn_readfirstlane(x1 + pix_floordiv(2 * dx * w + S, 2 * S));
        y1 = __builtin_amdgcn_readfirstlane(y1 + pix_floordiv(2 * dy * h + S, 2 * S));
        if (pix_outside(x1, y1, x1 + w - 1, y1 + h - 1, H, W)) break;
        if (tid == 0) {
            float *r = trk + (int64_t)g * 5;
            r[0] = (float)(x1 + 1); r[1] = (float)(y1 + 1); r[2] = (float)(x1 + w); r[3] = (float)(y1 + h); r[4] = conf;
        }
        n = s;
        if constexpr (ADAPT) {
            // The template update.  Every condition below is block-uniform: ad and conf are, c0 is read by every thread from
            // the same LDS slots.  (conf < update_conf skips the guard: it could not change the decision.)
            if (ad.a > 0 && conf >= ad.update_conf) {
                // P, the window that won: cells dx .. dx+S-1 by dy .. dy+S-1 of the winner's level box on frame g.  It is in
                // sreg, at row R+dy and byte R+dx of the region, when the winner's level is ns, the one the loop gathered last
                // (a winner was admissible); otherwise -- also when level ns was skipped -- the S x S window is gathered again
                // at the head of sreg (pitch tq, byte shift 0).
                const int udy = __builtin_amdgcn_readfirstlane(dy), udx = __builtin_amdgcn_readfirstlane(dx);
                const int lwin = __builtin_amdgcn_readfirstlane((int)((uint32_t)key & 7u) - kPixMaxScales);
                int pbase = (udy + R) * pitch + ((udx + R) >> 2), ppitch = pitch, psh = (udx + R) & 3;
                if (lwin != ns) {
                    // (the winner's level box before the move: the move, taken back)
                    const int bx1 = x1 - pix_floordiv(2 * udx * w + S, 2 * S), by1 = y1 - pix_floordiv(2 * udy * h + S, 2 * S);
                    // Hazards of the re-gather: the tables' last readers (the last level's gather) and sreg's last readers
                    // (the last level's SAD pass) are behind the barrier of the key reduction above, which every thread has
                    // passed; the barrier behind the tables orders them before the gather, the one behind the gather orders
                    // sreg before the reads of P below.
                    if constexpr (BOX) {
                        pix_tables_box(tcol, tcolb, trow, trowb, bx1, by1, w, h, S, udx, udy, S, H, W);
                        __syncthreads();
                        pix_gather_box(sreg, tq, tcol, tcolb, trow, trowb, S, integ + (int64_t)g * frame_cells, W + 1);
                    } else {
                        pix_tables(tcol, trow, bx1, by1, w, h, S, udx, udy, S, H, W);
                        __syncthreads();
                        pix_gather(sreg, tq, tcol, trow, S, a.images + (int64_t)g * frame_bytes, W);
                    }
                    __syncthreads();
                    pbase = 0;
                    ppitch = tq;
                    psh = 0;
                }
                // the guard: SAD0 = sum |Tm0 - P|, every thread over the cells it owns, then over the block
                uint32_t pw[kPixOwn], sad0 = 0;
#pragma unroll
                for (int k = 0; k < kPixOwn; ++k) {
                    const int d = tid + k * kPixLT;
                    pw[k] = 0;
                    if (d < S * tq) {
                        const int i = d / tq, o = pbase + i * ppitch + (d - i * tq);
                        const uint32_t lo = sreg[o], hi = psh ? sreg[o + 1] : 0u;       // (o + 1: the row's spare dword at most)
                        pw[k] = __builtin_amdgcn_alignbyte(hi, lo, psh);
                        sad0 = __builtin_amdgcn_sad_u8(tm0[k], pw[k], sad0);
                    }
                }
#pragma unroll
                for (int d = 32; d > 0; d >>= 1) sad0 += __shfl_xor(sad0, d, 64);
                // ssad0 is single-buffered: its readers of the last accepted-or-refused update are behind the barriers of
                // this step's tables and gather
                if (lane == 0) ssad0[wv] = sad0;
                __syncthreads();
                sad0 = ssad0[0];
#pragma unroll
                for (int k = 1; k < kPixWaves; ++k) sad0 += ssad0[k];
                const float c0 = 1.0f - (float)sad0 / denom;
                if (c0 >= ad.drift_conf) {
                    // A = ((256 - a) * A + a * (P << 8) + 128) >> 8 on the cells the thread owns, and Tm = (A + 128) >> 8 into
                    // its own dwords of stm.  Hazards: the last SAD pass that read stm is behind the barrier of the key
                    // reduction (and the guard's); the next step's SAD pass is behind the two barriers of its tables and
                    // gather, which follow these writes.
                    const uint32_t wa = (uint32_t)ad.a, wk = 256u - wa;
#pragma unroll
                    for (int k = 0; k < kPixOwn; ++k) {
                        const int d = tid + k * kPixLT;
                        if (d < S * tq) {
                            uint32_t tmv = 0;
#pragma unroll
                            for (int b = 0; b < 4; ++b) {
                                const int sft = 16 * (b & 1);
                                uint32_t &pair = acc[2 * k + (b >> 1)];
                                const uint32_t av = (pair >> sft) & 0xFFFFu, pv = (pw[k] >> (8 * b)) & 0xFFu;
                                const uint32_t nv = (wk * av + wa * (pv << 8) + 128u) >> 8;      // <= 256 * 65280 + 128
                                pair = (pair & ~(0xFFFFu << sft)) | (nv << sft);
                                tmv |= ((nv + 128u) >> 8) << (8 * b);
                            }
                            stm[d] = tmv;
                        }
                    }
                }
            }
        }
    }
    // the rows of this half the chain did not write: beyond its end, and the frames a step > 1 skips
    const int nf = dir > 0 ? F - 1 - af : af;         // frames of the half, at distance 1 .. nf from the anchor
    for (int64_t i = tid; i < (int64_t)nf * 5; i += kPixLT) {
        const int d = (int)(i / 5) + 1, e = (int)(i - (int64_t)(d - 1) * 5);
        if (d % a.step == 0 && d / a.step <= n) continue;
        trk[(int64_t)(af + dir * d) * 5 + e] = qnan;
    }
}

// grid (C*T, 2): blockIdx.y = 0 tracks forward (and owns the slot's anchor row, its anchors entry, a dead slot's rows and --
// slot 0 of a class -- the class's ntracks), 1 backward.  The body of track_pixels_kernel and track_pixels_scaled_kernel.
template <bool SCALED, bool BOX = false, bool ADAPT = false>
__device__ __forceinline__ void pix_slots_body(const PixTrackArgs &a, const PixScaleArgs sc,
                                               const PixAdaptArgs ad = PixAdaptArgs{0, 0.0f, 0.0f})
{
    __shared__ int snt;
    const int tid = threadIdx.x;
    const int64_t slot = blockIdx.x;
    const int c = (int)(slot / a.T), t = (int)(slot - (int64_t)c * a.T);
    const int dir = blockIdx.y == 0 ? 1 : -1;
    const int F = a.F;
    float *trk = a.tracks + slot * F * 5;

    int4 ab = make_int4(0, 0, 0, 0);
    const int state = pix_anchor_state(a, slot, ab);
    const bool live = state == 1;
    const int af = live ? a.aframes[slot] - 1 : 0;

    if (dir > 0) {
        if (tid == 0) {
            if (state < 0) atomicOr(a.status, kStBadPixAnchor);
            a.anchors[slot * 3] = (float)a.aframes[slot];
            a.anchors[slot * 3 + 1] = -1.0f;
            a.anchors[slot * 3 + 2] = a.ascores ? a.ascores[slot] : 0.0f;
        }
        if (t == 0) {            // (block-uniform) the class's count: 1 + its last live slot
            if (tid == 0) snt = 0;
            __syncthreads();
            for (int k = tid; k < a.T; k += kPixLT) {
                int4 bk;
                if (pix_anchor_state(a, (int64_t)c * a.T + k, bk) == 1) atomicMax(&snt, k + 1);
            }
            __syncthreads();
            if (tid == 0) a.ntracks[c] = snt;
        }
    }
    if (!live) {                 // every row of a dead slot is the forward block's
        if (dir > 0) pix_no_rows(trk, F);
        return;
    }
    if constexpr (ADAPT) pix_chain<SCALED, BOX, true>(a, trk, af, ab, dir, sc, ad);
    else pix_chain<SCALED, BOX>(a, trk, af, ab, dir, sc);
}

__global__ __launch_bounds__(kPixLT) void track_pixels_kernel(const PixTrackArgs a)
{
    pix_slots_body<false>(a, PixScaleArgs{0, 1, 0});
}

// vdet_track_pixels_scaled: the same launch with the scale search in every chain
__global__ __launch_bounds__(kPixLT) void track_pixels_scaled_kernel(const PixTrackArgs a, const PixScaleArgs sc)
{
    pix_slots_body<true>(a, sc);
}

// vdet_track_pixels_box: the same launch with box sampling in every chain (a.images: the integral); sc.ns = 0: the fixed scale
__global__ __launch_bounds__(kPixLT) void track_pixels_box_kernel(const PixTrackArgs a, const PixScaleArgs sc)
{
    pix_slots_body<true, true>(a, sc);
}

// The tracker launch of the greedy loop (vdet_track_volume_pixels): grid (C, 2), one block per class and direction.  The anchor
// is the one track_pick_kernel left in the class's TrackState -- frame anchor_frame, box boxes[anchor_frame, anchor_box]
// truncated toward zero (vdet/track.py:224, map(int, bbox)) --, the tubelet goes into slot ntracks of the class, every row of
// which this launch writes exactly once.  A class that is not active returns at once.  An anchor that cannot be tracked
// (pix_box_state) latches kStBadPixAnchor and leaves a slot of NaN rows: the loop goes on and nothing is suppressed by it.
// Reads of a: what pix_chain reads.  The body of track_pixel_chain_kernel and track_pixel_chain_scaled_kernel.
template <bool SCALED, bool BOX = false, bool ADAPT = false>
__device__ __forceinline__ void pix_greedy_body(const PixTrackArgs &a, const PixScaleArgs sc, const TrackState *__restrict__ st,
                                                const float *__restrict__ boxes, int B, int max_tracks, float *__restrict__ tracks,
                                                int *status, const PixAdaptArgs ad = PixAdaptArgs{0, 0.0f, 0.0f})
{
    const int c = blockIdx.x;
    const int dir = blockIdx.y == 0 ? 1 : -1;
    const TrackState s = st[c];
    if (!s.active) return;
    float *trk = tracks + ((int64_t)c * max_tracks + s.ntracks) * a.F * 5;
    int4 ab = make_int4(0, 0, 0, 0);
    if (pix_box_state(boxes + ((int64_t)s.anchor_frame * B + s.anchor_box) * 4, a.H, a.W, ab) < 0) {
        if (dir > 0) {
            if (threadIdx.x == 0) atomicOr(status, kStBadPixAnchor);
            pix_no_rows(trk, a.F);
        }
        return;
    }
    if constexpr (ADAPT) pix_chain<SCALED, BOX, true>(a, trk, s.anchor_frame, ab, dir, sc, ad);
    else pix_chain<SCALED, BOX>(a, trk, s.anchor_frame, ab, dir, sc);
}

__global__ __launch_bounds__(kPixLT) void track_pixel_chain_kernel(const PixTrackArgs a, const TrackState *__restrict__ st,
                                                                   const float *__restrict__ boxes, int B, int max_tracks,
                                                                   float *__restrict__ tracks, int *status)
{
    pix_greedy_body<false>(a, PixScaleArgs{0, 1, 0}, st, boxes, B, max_tracks, tracks, status);
}

// vdet_track_volume_pixels_scaled: the same launch with the scale search in the chain
__global__ __launch_bounds__(kPixLT) void track_pixel_chain_scaled_kernel(const PixTrackArgs a, const PixScaleArgs sc,
                                                                          const TrackState *__restrict__ st,
                                                                          const float *__restrict__ boxes, int B, int max_tracks,
                                                                          float *__restrict__ tracks, int *status)
{
    pix_greedy_body<true>(a, sc, st, boxes, B, max_tracks, tracks, status);
}

// vdet_track_volume_pixels_box: the same launch with box sampling in the chain (a.images: the integral)
__global__ __launch_bounds__(kPixLT) void track_pixel_chain_box_kernel(const PixTrackArgs a, const PixScaleArgs sc,
                                                                       const TrackState *__restrict__ st,
                                                                       const float *__restrict__ boxes, int B, int max_tracks,
                                                                       float *__restrict__ tracks, int *status)
{
    pix_greedy_body<true, true>(a, sc, st, boxes, B, max_tracks, tracks, status);
}

// vdet_track_pixels_adaptive / vdet_track_volume_pixels_adaptive: the same launches with the template update in every chain, for
// point sampling (a.images: the images) and box sampling (a.images: the integral); sc.ns = 0: the fixed scale
__global__ __launch_bounds__(kPixLT) void track_pixels_adaptive_kernel(const PixTrackArgs a, const PixScaleArgs sc, const PixAdaptArgs ad)
{
    pix_slots_body<true, false, true>(a, sc, ad);
}

__global__ __launch_bounds__(kPixLT) void track_pixels_adaptive_box_kernel(const PixTrackArgs a, const PixScaleArgs sc,
                                                                           const PixAdaptArgs ad)
{
    pix_slots_body<true, true, true>(a, sc, ad);
}

__global__ __launch_bounds__(kPixLT) void track_pixel_chain_adaptive_kernel(const PixTrackArgs a, const PixScaleArgs sc,
                                                                            const PixAdaptArgs ad, const TrackState *__restrict__ st,
                                                                            const float *__restrict__ boxes, int B, int max_tracks,
                                                                            float *__restrict__ tracks, int *status)
{
    pix_greedy_body<true, false, true>(a, sc, st, boxes, B, max_tracks, tracks, status, ad);
}

__global__ __launch_bounds__(kPixLT) void track_pixel_chain_adaptive_box_kernel(const PixTrackArgs a, const PixScaleArgs sc,
                                                                                const PixAdaptArgs ad,
                                                                                const TrackState *__restrict__ st,
                                                                                const float *__restrict__ boxes, int B, int max_tracks,
                                                                                float *__restrict__ tracks, int *status)
{
    pix_greedy_body<true, true, true>(a, sc, st, boxes, B, max_tracks, tracks, status, ad);
}

// ---- the integral image of the luma (vdet_luma_integral): uint8 [F,H,W,3] -> uint32 [F,H+1,W+1], two launches that between
// them write every element once (rows: columns 0 .. W of the rows 1 .. H; cols: row 0, then rows 1 .. H in place)
constexpr int kPixIntRowLT = 256, kPixIntRowWaves = kPixIntRowLT / 64;       // a wave per image row
constexpr int kPixIntColLT = 128, kPixIntColDepth = 8;

// grid ceil(F*H / 4): wave r of the launch scans image row r (frame r / H, row r % H) into I[f, y+1, :]
__global__ __launch_bounds__(kPixIntRowLT) void luma_integral_rows_kernel(const uint8_t *__restrict__ images, int64_t nrows, int H, int W,
                                                                          uint32_t *__restrict__ integ)
{
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * kPixIntRowWaves + (threadIdx.x >> 6);
    if (row >= nrows) return;                // (the whole wave; no barrier below)
    const int64_t f = row / H;
    const int y = (int)(row - f * H);
    const uint8_t *src = images + row * W * 3;
    uint32_t *dst = integ + (f * (H + 1) + y + 1) * (int64_t)(W + 1);
    if (lane == 0) dst[0] = 0;
    uint32_t carry = 0;                      // the sum of the trips so far
    for (int x0 = 0; x0 < W; x0 += 64) {     // (wave-uniform)
        const int x = x0 + lane;
        uint32_t v = x < W ? pix_luma(src + 3 * x) : 0u;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t u = __shfl_up(v, d, 64);
            if (lane >= d) v += u;
        }
        v += carry;
        if (x < W) dst[x + 1] = v;
        carry = __shfl(v, 63, 64);
    }
}

// grid F * ceil((W+1) / 128): a thread per column of a frame's table
__global__ __launch_bounds__(kPixIntColLT) void luma_integral_cols_kernel(uint32_t *__restrict__ integ, int H, int W, int nbx)
{
    const int64_t f = blockIdx.x / nbx;
    const int x = (int)(blockIdx.x - f * nbx) * kPixIntColLT + threadIdx.x;
    if (x > W) return;
    const int64_t pw = W + 1;
    uint32_t *p = integ + f * (H + 1) * pw + x;
    p[0] = 0;
    uint32_t acc = 0;
    int y = 1;
    for (; y + kPixIntColDepth - 1 <= H; y += kPixIntColDepth) {
        uint32_t v[kPixIntColDepth];
#pragma unroll
        for (int k = 0; k < kPixIntColDepth; ++k) v[k] = p[(y + k) * pw];
#pragma unroll
        for (int k = 0; k < kPixIntColDepth; ++k) {
            acc += v[k];
            p[(y + k) * pw] = acc;
        }
    }
    for (; y <= H; ++y) {
        acc += p[y * pw];
        p[y * pw] = acc;
    }
}

}  // namespace vdet
