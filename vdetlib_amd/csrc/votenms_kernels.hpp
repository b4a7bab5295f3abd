// Bounding-box voting (Gidaris & Komodakis, ICCV 2015) on the per-frame detection lists of tracknms_kernels.hpp: the hard NMS of
// vdet_nms_tracks decides which rows are kept, in which order and with what score; every kept row's BOX then becomes the
// weighted mean of the boxes of the list's present rows that overlap it -- the rows the NMS threw away included.  Semantics in
// full: include/vdet_hip.h (vdet_vote_nms_tracks); the rule in numpy: tests/votenms_spec.py, which the kernel equals on bits.
//
// The LIST, the hard selection and the launch shape are tracknms_kernels.hpp's, through its shared pieces: tn_open, TnLds,
// tn_load_row, tn_select, tn_store_row / tn_store_pad, tn_close.
//
// Per wave, LDS: box [n] float4, COMPOSITE [n] 64-bit, f32 score [n], rank -> row index [n] int32, n = top_still + T of THE CALL
// (32 bytes per candidate, softnms_kernel's: 4 waves up to 511 candidates, 2 up to 1023, 1 at the limit of 1024).
//   composite: tracknms_kernel's (score_key << 32 | j alive, rank + 1 kept, 0 absent or suppressed).
//   score:     the f32 score the NMS orders by, NaN for an absent row.  The composite of a suppressed row is zeroed, so the score
//              is what still tells it from an absent one, and it is the 'score' weight.
//   rank -> row: written by the lane that marks a row kept; there are never more kept rows than candidates.
// The areas are not stored: box_area of the stored box, as the selection of tracknms_kernel computes them, so the table above
// takes the four bytes and the waves-per-workgroup breaks stay where softnms_kernel has them.
// SELECTION: tn_select, the one loop tracknms_kernel runs, with the table entry as its on_keep.  The kept set, its order and the
// zero-union flag of the pairs it evaluates are that kernel's.
// VOTING pass, after it: LANE l takes the ranks l, l + 64, ... below min(kept, R), holds that row's box in registers and walks
// the rows 0 .. n-1 of the list from LDS -- every lane reads the same address: a broadcast -- testing each present row with
// pair_pred at the vote threshold (the row itself votes untested) and adding w and w * x1, y1, x2, y2 to five float64 registers.
// That IS the rule's sum: sequential, ascending row index, from 0.0, one rounded multiply and one rounded add per step (the TU is
// built with -ffp-contract=off).  No shuffles, no atomics.  The zero-union bit of pair_pred is ignored here: such a row is not
// a voter and nothing is latched, these are not pairs the reference evaluates.  The lane then divides (correctly rounded f64
// divisions), and writes rank row r of every output itself; the ranks behind the count are filled as in tracknms_kernel.
// Cost: kept x ceil(n / 64) pair tests per lane for the selection plus ceil(min(kept, R) / 64) x n for the voting.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tracknms_kernels.hpp"  // TrackNmsArgs, TnList, TnRow, the shared pieces, kTnMaxList

namespace vdet {

constexpr int kVnBytesPerCand = 32;  // float4 box + 64-bit composite + f32 score + int32 rank -> row entry
constexpr int kVnScore = 0, kVnUniform = 1;

struct VoteNmsArgs {
    TrackNmsArgs tn;            // the list sources and the outputs of vdet_nms_tracks; tn.otracks[..., :4] = the voted box
    float *obox0;               // [C,R,F,4] the row's own box
    int32_t *ovotes;            // [C,R,F] voters, the row itself included
    int weights;
    float v32;                  // thresh_to_f32(vote_thresh)
};

__device__ __forceinline__ bool vn_finite(double x) { return (x - x) == 0.0; }

__global__ __launch_bounds__(256) void votenms_kernel(const VoteNmsArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char vn_smem[];
    const TrackNmsArgs &g = a.tn;
    const int lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    TnList m;
    bool badkeep = false;
    if (!tn_open(g, nw, w, m, badkeep)) return;
    const TnLds lds(vn_smem, nw, w, g.nmax);
    float4 *sbox = lds.box();
    unsigned long long *scomp = lds.comp();
    float *sscore = lds.plane<float>(0);
    int *srow = lds.plane<int>(1);

    const float qnan = __uint_as_float(0x7FC00000u);
    // gather (tracknms_kernel's, plus the score: NaN marks an absent row, whose box is never read)
    unsigned long long best = 0ull;
    for (int j = lane; j < m.n; j += 64) {
        TnRow r;
        unsigned long long k = 0ull;
        float sj = qnan;
        if (tn_load_row(g, m, j, r, badkeep)) {
            sbox[j] = r.box;
            sj = r.s32;
            k = ((unsigned long long)score_key(r.s32) << 32) | (unsigned)j;
        }
        sscore[j] = sj;
        scomp[j] = k;
        best = k > best ? k : best;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();

    bool zero = false;
    const int kept = tn_select(g, m, lane, sbox, scomp, best, zero, [srow](int rank, int j) { srow[rank] = j; });
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();

    // voting and output: one lane per kept row, the rows of the list in ascending index
    const int live = kept < g.R ? kept : g.R;
    const bool uniform = a.weights == kVnUniform;
    for (int r = lane; r < live; r += 64) {
        const int i = srow[r];                           // (r < kept <= n: written above)
        const float4 bi = sbox[i];
        const float ai = box_area(bi);
        double sw = 0.0, sx = 0.0, sy = 0.0, sz = 0.0, st = 0.0;
        int votes = 0;
        for (int j = 0; j < m.n; ++j) {
            const float sj = sscore[j];
            if (sj != sj) continue;                      // absent
            const float4 bj = sbox[j];
            if (j != i && !(pair_pred(bi, ai, bj, box_area(bj), a.v32) & 1u)) continue;
            const double wj = uniform ? 1.0 : (sj > 0.0f ? (double)sj : 0.0);
            sw += wj;
            sx += wj * (double)bj.x;
            sy += wj * (double)bj.y;
            sz += wj * (double)bj.z;
            st += wj * (double)bj.w;
            ++votes;
        }
        float4 bv = bi;
        if (sw > 0.0) {
            const double qx = sx / sw, qy = sy / sw, qz = sz / sw, qt = st / sw;
            if (vn_finite(qx) && vn_finite(qy) && vn_finite(qz) && vn_finite(qt))
                bv = make_float4((float)qx, (float)qy, (float)qz, (float)qt);
        }
        TnRow row;
        bool dummy = false;
        tn_load_row(g, m, i, row, dummy);                // the source's own score and src (the lines are in cache)
        const int64_t e = m.obase + (int64_t)r * m.F;
        tn_store_row(g, e, bv, row.s32, row.s64, row.src);
        float *o0 = a.obox0 + e * 4;
        o0[0] = bi.x; o0[1] = bi.y; o0[2] = bi.z; o0[3] = bi.w;
        a.ovotes[e] = votes;
    }
    for (int r = live + lane; r < g.R; r += 64) {
        const int64_t e = m.obase + (int64_t)r * m.F;
        tn_store_pad(g, e);
        float *o0 = a.obox0 + e * 4;
        o0[0] = qnan; o0[1] = qnan; o0[2] = qnan; o0[3] = qnan;
        a.ovotes[e] = 0;
    }
    tn_close(g, m, lane, kept, badkeep, zero);
}

}  // namespace vdet

