// Motion-guided propagation of detections: a dense block-motion field per frame pair, and boxes moved along it to the frames
// around them (the stage T-CNN runs between the still-image detector and per-frame NMS / tubelet seeding).  The rule is
// tests/motion_spec.py, integers on uint8 pixels; the device matches it bit for bit.
//
//   field     direction 0 is f -> f+1, direction 1 is f -> f-1; block (by,bx) of P x P pixels of frame f against frame g: every
//             (dy,dx) in [-R,R]^2 gets SAD = sum |L_f[cy(by*P+i), cx(bx*P+j)] - L_g[cy(by*P+i+dy), cx(bx*P+j+dx)]| with cx, cy
//             clamped to the image (edge replication, also of the partial blocks); the smallest key (SAD, dy^2+dx^2, dy, dx)
//             wins; field = (dx,dy) int16, cost = SAD; the frame without a partner is zero
//   table     fsum[d,f,y,x,:] = sum of field[d,f,r,c,:] over r < y, c < x, int32 [2,F,Hb+1,Wb+1,2]
//   box       moves by the mean (rounded half up) of the vectors of the blocks whose centre pixel lies in it: four entries of
//             fsum per component
//
// motion_match_kernel<P>: ONE launch over every tile of every frame in both directions.  A workgroup owns a 64 x 64 pixel tile
// of one (direction, frame): (64/P)^2 neighbouring blocks that share one region of frame g in LDS.
//   1. the clamped column / row tables of the tile (frame f) and of its region (frame g, R more on every side);
//   2. two gathers (pix_gather, the tracker's): luma from the three bytes in flight, four pixels to a dword of LDS;
//   3. a block belongs to a group of gw lanes of one wave (gw = 16, 32 or 64, the host's choice: the one that wastes the fewest
//      lanes on (2R+1)^2 candidates); a candidate is P*P/4 v_sad_u8 on dwords that v_alignbyte_b32 cuts from two neighbouring
//      region dwords, as in track_pixels_kernel (the template dword is one address per group: an LDS broadcast);
//   4. the key packed in 64 bits (SAD | dy^2+dx^2 | dy+R | dx+R) is min-reduced by wave shuffles inside the group; keys are
//      unique, so the order cannot matter; the group's first lane stores the vector (one dword) and the cost.
// LDS: region 96 x 25 dwords (one spare dword per row for the pair read at shift 0) + tile 64 x 16 dwords + tables: 14.6 KiB,
// static.  Every element of field and cost is written by this launch (a tile of a frame without a partner stores zeros).
//
// motion_table_kernel: one launch, a wave per (direction, frame).  Lanes own 64 neighbouring columns and run down the rows with
// the column sums in registers; a row is finished by a wave scan and the carry of the columns to the left, which the wave left
// in LDS (a slot per row) when it did the 64 columns before.  Every element of fsum, row 0 and column 0 included, is stored
// once; nothing is read back from memory.
//
// propagate_boxes_kernel: ONE launch, a thread per (class, direction, list entry j, source frame) with the FRAME innermost, so
// that at step m neighbouring lanes write neighbouring frames of one slot of [C,T,F,5].  A thread walks its reach steps and
// writes one row per step: the moved box on frame g = f +- m, or -- the chain has ended, the entry does not exist, the data is
// bad -- a NaN row; a step that leaves the video writes the NaN row of the frame (g mod F), whose own source frame lies outside
// the video, so every row of every slot is stored exactly once.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pixtrack_kernels.hpp"

namespace vdet {

constexpr int kStBadPropagate = 8192;    // vdet_propagate_boxes: a keep_cnt / keep_idx out of range or a source box that cannot be moved
constexpr int kMoLT = 256, kMoWaves = kMoLT / 64;
constexpr int kMoTile = 64;              // tile side in pixels
constexpr int kMoMaxR = 16, kMoMaxReach = 16;
constexpr int kMoMaxReg = kMoTile + 2 * kMoMaxR;        // region side
constexpr int kMoMaxPitch = kMoMaxReg / 4 + 1;          // region row pitch in dwords (one spare: see the pair read)
constexpr int kMoTilePitch = kMoTile / 4;
constexpr int kMoTabRows = 4096;         // block rows of a frame: ceil(32767 / 8)
constexpr int kMoTabDepth = 4;           // rows whose loads are in flight together
constexpr int kMoPropLT = 256;
static_assert(kMoLT == kPixLT && kMoMaxReg <= kPixMaxP, "pix_gather runs kPixLT threads over at most kPixMaxP cells a side");

struct MotionArgs {
    const uint8_t *images;      // [F,H,W,3]
    int F, H, W, R;
    int Hb, Wb;                 // blocks per column / row of a frame
    int ty, tx;                 // tiles per column / row of a frame
    int gw;                     // lanes per block: 16, 32 or 64; (64/P)^2 is a multiple of kMoWaves * 64 / gw
    uint32_t *field;            // [2,F,Hb,Wb] (dx | dy << 16), the int16 pairs
    int32_t *cost;              // [2,F,Hb,Wb]
};

__device__ __forceinline__ int mo_clamp(int v, int hi)      // to 0..hi
{
    return v < 0 ? 0 : (v > hi ? hi : v);
}

template <int P>
__global__ __launch_bounds__(kMoLT) void motion_match_kernel(const MotionArgs a)
{
    constexpr int NB = kMoTile / P, NBLK = NB * NB, TQ = P / 4;
    __shared__ uint32_t sreg[kMoMaxReg * kMoMaxPitch];
    __shared__ uint32_t stm[kMoTile * kMoTilePitch];
    __shared__ int tcolT[kMoTile], trowT[kMoTile], tcolR[kMoMaxReg], trowR[kMoMaxReg];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int F = a.F, H = a.H, W = a.W, R = a.R, Hb = a.Hb, Wb = a.Wb;
    const int ntile = a.ty * a.tx;
    const int64_t df = blockIdx.x / ntile;
    const int tile = (int)(blockIdx.x - df * ntile);
    const int dir = (int)(df / F), f = (int)(df - (int64_t)dir * F);
    const int tyi = tile / a.tx, txi = tile - tyi * a.tx;
    const int by0 = tyi * NB, bx0 = txi * NB;
    const int g = dir == 0 ? f + 1 : f - 1;
    const int64_t obase = df * Hb * Wb;
    if (g < 0 || g >= F) {                       // (block-uniform) the frame without a partner
        if (tid < NBLK) {
            const int bi = tid / NB, bj = tid - bi * NB;
            if (by0 + bi < Hb && bx0 + bj < Wb) {
                const int64_t o = obase + (int64_t)(by0 + bi) * Wb + bx0 + bj;
                a.field[o] = 0u;
                a.cost[o] = 0;
            }
        }
        return;
    }
    const int n = kMoTile + 2 * R, pitch = n / 4 + 1;
    // 1. the tables: tile columns, tile rows, region columns, region rows (tcol = 3 * column)
    for (int i = tid; i < 2 * kMoTile + 2 * n; i += kMoLT) {
        if (i < kMoTile) tcolT[i] = 3 * mo_clamp(bx0 * P + i, W - 1);
        else if (i < 2 * kMoTile) trowT[i - kMoTile] = mo_clamp(by0 * P + i - kMoTile, H - 1);
        else if (i < 2 * kMoTile + n) tcolR[i - 2 * kMoTile] = 3 * mo_clamp(bx0 * P - R + i - 2 * kMoTile, W - 1);
        else trowR[i - 2 * kMoTile - n] = mo_clamp(by0 * P - R + i - 2 * kMoTile - n, H - 1);
    }
    __syncthreads();
    // 2. the tile of frame f and its region of frame g
    const int64_t frame_bytes = (int64_t)H * W * 3;
    pix_gather(stm, kMoTilePitch, tcolT, trowT, kMoTile, a.images + (int64_t)f * frame_bytes, W);
    pix_gather(sreg, pitch, tcolR, trowR, n, a.images + (int64_t)g * frame_bytes, W);
    __syncthreads();
    // 3. + 4. a block per group of gw lanes, kMoWaves * 64 / gw blocks a round
    const int side = 2 * R + 1, ncand = side * side;
    const int gw = a.gw, ng = 64 / gw;
    const int grp = lane / gw, gl = lane - grp * gw;
    for (int b0 = 0; b0 < NBLK; b0 += kMoWaves * ng) {
        const int b = b0 + wv * ng + grp;
        const int bi = b / NB, bj = b - bi * NB;
        const bool live = by0 + bi < Hb && bx0 + bj < Wb;
        unsigned long long key = ~0ull;
        if (live) {
            for (int cand = gl; cand < ncand; cand += gw) {
                const int cy = cand / side, cx = cand - cy * side;      // dy + R, dx + R
                const int byte0 = bj * P + cx, sh = byte0 & 3;
                const uint32_t *rrow = sreg + (bi * P + cy) * pitch + (byte0 >> 2);
                const uint32_t *tp = stm + bi * P * kMoTilePitch + bj * TQ;
                uint32_t sad = 0;
                for (int i = 0; i < P; ++i) {
                    uint32_t lo = rrow[0];
#pragma unroll
                    for (int q = 0; q < TQ; ++q) {
                        const uint32_t hi = rrow[q + 1];
                        sad = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(hi, lo, sh), tp[q], sad);
                        lo = hi;
                    }
                    rrow += pitch;
                    tp += kMoTilePitch;
                }
                const int dy = cy - R, dx = cx - R;
                const unsigned long long k = ((unsigned long long)sad << 32) | ((unsigned long long)(dy * dy + dx * dx) << 16) |
                                             ((unsigned long long)cy << 8) | (unsigned long long)cx;
                key = k < key ? k : key;
            }
        }
        for (int d = gw >> 1; d > 0; d >>= 1) {          // (every lane of the wave: the groups never mix below gw)
            const unsigned long long k2 = __shfl_xor(key, d, 64);
            key = k2 < key ? k2 : key;
        }
        if (live && gl == 0) {
            const int dy = (int)((key >> 8) & 0xFF) - R, dx = (int)(key & 0xFF) - R;
            const int64_t o = obase + (int64_t)(by0 + bi) * Wb + bx0 + bj;
            a.field[o] = ((uint32_t)dx & 0xFFFFu) | ((uint32_t)dy << 16);
            a.cost[o] = (int32_t)(key >> 32);
        }
    }
}

// grid 2 * F, one wave each: field (int16 pairs) [2*F,Hb,Wb] -> fsum (int32 pairs) [2*F,Hb+1,Wb+1].  |component| <= 16 and
// Hb * Wb <= 2^24: the sums stay below 2^28
__global__ __launch_bounds__(64) void motion_table_kernel(const uint32_t *__restrict__ field, int Hb, int Wb, int2 *__restrict__ fsum)
{
    __shared__ int2 scar[kMoTabRows];            // per row: the sum over the columns left of the 64 in hand
    const int lane = threadIdx.x;
    const uint32_t *fld = field + (int64_t)blockIdx.x * Hb * Wb;
    const int64_t pw = Wb + 1;
    int2 *out = fsum + (int64_t)blockIdx.x * (Hb + 1) * pw;
    for (int x = lane; x <= Wb; x += 64) out[x] = make_int2(0, 0);
    for (int x0 = 0; x0 < Wb; x0 += 64) {        // (wave-uniform)
        const int x = x0 + lane;
        const bool in = x < Wb;
        int ax = 0, ay = 0;                      // the column's sums down to the row in hand
        for (int y0 = 0; y0 < Hb; y0 += kMoTabDepth) {
            uint32_t v[kMoTabDepth];
#pragma unroll
            for (int k = 0; k < kMoTabDepth; ++k) v[k] = in && y0 + k < Hb ? fld[(int64_t)(y0 + k) * Wb + x] : 0u;
#pragma unroll
            for (int k = 0; k < kMoTabDepth; ++k) {
                const int y = y0 + k;
                if (y >= Hb) break;              // (wave-uniform)
                ax += (int)(int16_t)(v[k] & 0xFFFFu);
                ay += (int)(int16_t)(v[k] >> 16);
                int sx = ax, sy = ay;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const int ux = __shfl_up(sx, d, 64), uy = __shfl_up(sy, d, 64);
                    if (lane >= d) { sx += ux; sy += uy; }
                }
                if (x0) {                        // (read by every lane before lane 63 replaces it: one wave, in order)
                    const int2 c = scar[y];
                    sx += c.x;
                    sy += c.y;
                }
                if (in) out[(y + 1) * pw + x + 1] = make_int2(sx, sy);
                if (x0 == 0 && lane == 0) out[(y + 1) * pw] = make_int2(0, 0);
                if (lane == 63) scar[y] = make_int2(sx, sy);
            }
        }
        __syncthreads();                         // (one wave: orders scar between two column passes)
    }
}

struct PropagateArgs {
    const int2 *fsum;           // [2,F,Hb+1,Wb+1]
    int F, Hb, Wb, P, H, W, B, C;
    const float *boxes;         // [F,B,4]
    const float *scores;        // [F,B,C]
    const int32_t *keep_idx;    // [F,C,kcap]
    const int32_t *keep_cnt;    // [F,C]
    int kcap, top, reach;
    float decay;
    float *tracks;              // [C,T,F,5], T = 2 * reach * top
    float *score;               // [C,T,F]
    int32_t *src;               // [C,T,F]
    int32_t *ntracks;           // [C]
    int *status;
};

// the blocks (of N on the axis) whose centre pixel P*b + P/2 lies in X1..X2; never empty
__device__ __forceinline__ void mo_block_range(int X1, int X2, int P, int N, int &a0, int &a1)
{
    const int h = P >> 1;
    a0 = -pix_floordiv(h - X1, P);
    a1 = pix_floordiv(X2 - h, P);
    if (a1 < a0) a0 = a1 = pix_floordiv(pix_floordiv(X1 + X2, 2), P);
    a0 = mo_clamp(a0, N - 1);
    a1 = mo_clamp(a1, N - 1);
    a1 = a1 < a0 ? a0 : a1;
}

// grid ceil(C * 2 * top * F / 256); |coordinate| <= 2^20 + 16 * 16 and n <= 2^24, |s| <= 2^28: everything stays in int32
__global__ __launch_bounds__(kMoPropLT) void propagate_boxes_kernel(const PropagateArgs a)
{
    const int64_t idx = (int64_t)blockIdx.x * kMoPropLT + threadIdx.x;
    const int F = a.F, top = a.top, reach = a.reach;
    if (idx >= (int64_t)a.C * 2 * top * F) return;
    const int f = (int)(idx % F);
    int64_t r = idx / F;
    const int j = (int)(r % top);
    r /= top;
    const int dir = (int)(r & 1), c = (int)(r >> 1);
    const int T = 2 * reach * top;
    if (f == 0 && j == 0 && dir == 0) a.ntracks[c] = T;
    // the source
    const int cnt = a.keep_cnt[(int64_t)f * a.C + c];
    bool bad = cnt < 0 || cnt > a.kcap, live = false;
    int b = 0;
    int4 ib = make_int4(0, 0, 0, 0);
    float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f, s = 0.f;
    if (!bad && j < cnt) {
        b = a.keep_idx[((int64_t)f * a.C + c) * a.kcap + j];
        if (b < 0 || b >= a.B) bad = true;
        else {
            const float *p = a.boxes + ((int64_t)f * a.B + b) * 4;
            const float lim = (float)kPixCoordMax;
            v0 = p[0]; v1 = p[1]; v2 = p[2]; v3 = p[3];
            // (a NaN fails every comparison, an infinity the bound)
            if (!(fabsf(v0) <= lim && fabsf(v1) <= lim && fabsf(v2) <= lim && fabsf(v3) <= lim)) bad = true;
            else {
                ib = make_int4((int)v0 - 1, (int)v1 - 1, (int)v2 - 1, (int)v3 - 1);
                s = a.scores[((int64_t)f * a.B + b) * a.C + c];
                live = true;
            }
        }
    }
    if (bad) atomicOr(a.status, kStBadPropagate);
    const int sgn = dir == 0 ? 1 : -1;
    const int64_t pw = a.Wb + 1, cells = (int64_t)(a.Hb + 1) * pw;
    const float qnan = __uint_as_float(0x7FC00000u);
    int Sx = 0, Sy = 0;
    for (int m = 1; m <= reach; ++m) {
        const int g = f + sgn * m;
        if (live) {
            if (g < 0 || g >= F) live = false;
            else {
                const int2 *fs = a.fsum + ((int64_t)dir * F + (g - sgn)) * cells;        // the frame the box is on
                int c0, c1, r0, r1;
                mo_block_range(ib.x + Sx, ib.z + Sx, a.P, a.Wb, c0, c1);
                mo_block_range(ib.y + Sy, ib.w + Sy, a.P, a.Hb, r0, r1);
                const int n = (c1 - c0 + 1) * (r1 - r0 + 1);
                const int2 q11 = fs[(r1 + 1) * pw + c1 + 1], q01 = fs[r0 * pw + c1 + 1], q10 = fs[(r1 + 1) * pw + c0], q00 = fs[r0 * pw + c0];
                Sx += pix_floordiv(2 * (q11.x - q01.x - q10.x + q00.x) + n, 2 * n);
                Sy += pix_floordiv(2 * (q11.y - q01.y - q10.y + q00.y) + n, 2 * n);
                if (pix_outside(ib.x + Sx, ib.y + Sy, ib.z + Sx, ib.w + Sy, a.H, a.W)) live = false;
            }
        }
        // the row of this step: frame g of slot (delta, j); a step beyond the video takes the row of frame g mod F of that
        // slot, whose own source frame lies outside the video
        const int di = sgn < 0 ? reach - m : reach + m - 1;
        int gw = g % F;
        gw = gw < 0 ? gw + F : gw;
        const int64_t o = ((int64_t)c * T + (int64_t)di * top + j) * F + gw;
        float *row = a.tracks + o * 5;
        if (live) {
            s = s * a.decay;
            const float fx = (float)Sx, fy = (float)Sy;
            row[0] = v0 + fx; row[1] = v1 + fy; row[2] = v2 + fx; row[3] = v3 + fy; row[4] = s;
            a.score[o] = s;
            a.src[o] = b;
        } else {
            row[0] = qnan; row[1] = qnan; row[2] = qnan; row[3] = qnan; row[4] = qnan;
            a.score[o] = qnan;
            a.src[o] = INT32_MIN;
        }
    }
}

}  // namespace vdet
