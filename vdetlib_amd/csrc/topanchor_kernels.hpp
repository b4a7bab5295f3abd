// Device anchor selection: the array form of protocol.top_detections / frame_top_detections (utils/protocol.py:330-351):
// per class the T best detections of a video (of every video of a batch, of every frame), in the [C,T] anchor tensors
// vdet_track_from_anchors reads.
//
// RULE.  A candidate of class c is a detection whose score is not NaN (and > thr, f32, with a threshold).  Candidates are
// ordered by (score descending, flat index f*B + b ascending), -0.0 == +0.0: slot t is the t-th one, slots behind the
// last candidate are empty.  With key = score_key(score) (0: not a candidate; no float has that key) the order is the
// order of the unique 64-bit records (key << 32 | ~index), so the T best of a class are one well-defined SET and the
// result cannot depend on the grid or on which workgroup runs first.
//
// SHAPE.  Selection by threshold, not by sort; scores [F,B,C] are read as they lie, a LANE PER CLASS (a wave reads 256
// contiguous bytes of a row), a wave per SEGMENT of kTopaRows consecutive rows which it walks in ascending order; no
// transposed or keyed copy exists.  A "video" is a frame range: the whole volume, a video of a batch (VidDesc table), or --
// frame mode -- every single frame.
//   1. four rounds of (topa_hist_kernel, topa_select_kernel): an 8-bit radix select, most significant byte first, finds
//      per (video, class) the key K of the T-th candidate and `need`, how many candidates with exactly that key lie inside
//      the cut.  The histograms are integer counts (LDS atomics per workgroup, then integer adds of the non-zero bins): sums
//      of integers do not depend on their order.  K = 0 when there are fewer than T candidates.
//   2. topa_count_kernel: per (video, segment, class) the number of keys > K and == K; topa_prefix_kernel turns them into
//      the exclusive prefix over the segments -- the write offset of the segment's records and how many records with key K
//      precede it.  The `need` candidates with key K of LOWEST flat index are the ones inside the cut: a segment, walking its
//      rows in ascending order, emits a key-K record iff fewer than `need` came before it.  No cursor, no atomic.
//   3. topa_gather_kernel writes the records (<= T per class) at those offsets; topa_emit_kernel, a workgroup per (video,
//      class), sorts them in LDS (bitonic, descending: the records are unique) and writes every slot of all four outputs,
//      the empty ones included, reading the score and the box of a slot from the caller's tensors (their bits are kept).
// Scratch: histogram V*C*256 words, counts V*segments*C*8 bytes, records V*C*T*8 bytes.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nms_kernels.hpp"       // score_key
#include "batch_kernels.hpp"     // VidDesc

namespace vdet {

constexpr int kTopaRows = 256;       // rows of a segment (one wave walks them in order): the row-chunk size
constexpr int kTopaHistLT = 1024;    // threads of topa_hist_kernel: 16 segments share one LDS histogram
constexpr int kTopaLT = 256;         // threads of the other kernels (count / gather: 4 segments per workgroup)
constexpr int kTopaMaxT = 1024;      // slots per class (the evaluator's tracks-per-class limit)
constexpr int kTopaMaxTFrame = 128;  // ... per frame in frame mode (vdet_det_nms_volume's top-k limit)

struct TopaArgs {
    const float *scores;         // [Ftot,B,C]
    const float4 *boxes;         // [Ftot,B]
    const VidDesc *vids;         // [V] or null: video v is frames [v*Fu, (v+1)*Fu)
    int Fu, V, B, C, T;
    int use_thr;
    float thr;
    int nseg;                    // segment slots per video (of the longest one)
    int frame_mode;              // frames are numbered in the volume, not in the "video" (which is one frame)
    uint32_t *hist;              // [V,C,256] zero between the rounds
    uint2 *state;                // [V,C] {key prefix, remaining rank} -> after round 4 {K, need}
    uint2 *cnt;                  // [V,nseg,C] {keys > K, keys == K} -> {record offset, key-K records before the segment}
    uint32_t *nrec;              // [V,C] records of the class
    unsigned long long *rec;     // [V,C,T]
    int64_t ovs, ocs;            // slot (v, c, t) is output element v*ovs + c*ocs + t
    int32_t *oframes;
    float4 *oboxes;
    float *oscores;
    int32_t *oindex;
};

__device__ __forceinline__ void topa_range(const TopaArgs &a, int v, int &f0, int &rows)
{
    f0 = a.vids ? a.vids[v].f0 : v * a.Fu;
    rows = (a.vids ? a.vids[v].F : a.Fu) * a.B;      // (< 2^31: host)
}

__device__ __forceinline__ uint32_t topa_key(const TopaArgs &a, float s)
{
    const bool cand = !(s != s) && (!a.use_thr || s > a.thr);
    return cand ? score_key(s) : 0u;
}

// The walk every pass shares: wave `seg` of video v, lane = class c; fn(key, local row) for its rows in ascending order,
// eight loads in flight.
template <typename Fn>
__device__ __forceinline__ void topa_walk(const TopaArgs &a, int f0, int rows, int seg, int c, Fn fn)
{
    const int r0 = seg * kTopaRows, r1 = min(rows, r0 + kTopaRows);
    const float *p = a.scores + ((int64_t)f0 * a.B + r0) * a.C + c;
    int r = r0;
    for (; r + 8 <= r1; r += 8, p += (int64_t)8 * a.C) {
        float s[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) s[k] = p[(int64_t)k * a.C];
#pragma unroll
        for (int k = 0; k < 8; ++k) fn(topa_key(a, s[k]), r + k);
    }
    for (; r < r1; ++r, p += a.C) fn(topa_key(a, *p), r);
}

// grid (ceil(nseg / 16), class tiles, V).  Round `pass` (0..3) counts byte 3 - pass of the keys that share the prefix found
// so far (round 0: of every key; the keys 0 of the non-candidates are the lowest bin of every round).
__global__ __launch_bounds__(kTopaHistLT) void topa_hist_kernel(const TopaArgs a, const int pass)
{
    __shared__ uint32_t lh[256 * 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int v = blockIdx.z, c0 = blockIdx.y * 64, c = c0 + lane;
    int f0, rows;
    topa_range(a, v, f0, rows);
    const int seg0 = blockIdx.x * (kTopaHistLT / 64);
    if ((int64_t)seg0 * kTopaRows >= rows) return;       // (block-uniform)
    for (int i = tid; i < 256 * 64; i += kTopaHistLT) lh[i] = 0u;
    __syncthreads();
    const int seg = seg0 + w;
    if (c < a.C && (int64_t)seg * kTopaRows < rows) {
        const int shift = 24 - 8 * pass;
        const uint32_t prefix = pass ? a.state[(int64_t)v * a.C + c].x : 0u;
        const uint32_t pmask = pass ? ~(0xFFFFFFFFu >> (8 * pass)) : 0u;
        topa_walk(a, f0, rows, seg, c, [&](uint32_t key, int) {
            if ((key & pmask) == prefix) atomicAdd(&lh[((key >> shift) & 255u) * 64 + lane], 1u);
        });
    }
    __syncthreads();
    for (int i = tid; i < 256 * 64; i += kTopaHistLT) {
        const uint32_t h = lh[i];
        const int cc = c0 + (i & 63);
        if (h && cc < a.C) atomicAdd(&a.hist[((int64_t)v * a.C + cc) * 256 + (i >> 6)], h);
    }
}

// grid (C, V), 256 threads: the bin of the round that holds the wanted rank; clears the histogram for the next round.
__global__ __launch_bounds__(256) void topa_select_kernel(const TopaArgs a, const int pass)
{
    __shared__ uint32_t sh[256];
    const int tid = threadIdx.x;
    const int64_t vc = (int64_t)blockIdx.y * a.C + blockIdx.x;
    const uint32_t h = a.hist[vc * 256 + tid];
    a.hist[vc * 256 + tid] = 0u;
    sh[tid] = h;
    const uint2 st = pass ? a.state[vc] : make_uint2(0u, (uint32_t)a.T);
    __syncthreads();
    uint32_t above = 0u;             // keys of the round in higher bins
    for (int b = tid + 1; b < 256; ++b) above += sh[b];
    const int shift = 24 - 8 * pass;
    if (above < st.y && st.y <= above + h) a.state[vc] = make_uint2(st.x | ((uint32_t)tid << shift), st.y - above);
    // fewer keys than the rank (T beyond the video's rows): bin 0, and the rank stays out of reach down to K = 0
    if (tid == 0 && above + h < st.y) a.state[vc] = make_uint2(st.x, st.y - above);
}

// grid (ceil(nseg / 4), class tiles, V)
__global__ __launch_bounds__(kTopaLT) void topa_count_kernel(const TopaArgs a)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int v = blockIdx.z, c = blockIdx.y * 64 + lane, seg = blockIdx.x * (kTopaLT / 64) + w;
    int f0, rows;
    topa_range(a, v, f0, rows);
    if (c >= a.C || (int64_t)seg * kTopaRows >= rows) return;
    const uint32_t K = a.state[(int64_t)v * a.C + c].x;
    uint32_t gt = 0u, eq = 0u;
    topa_walk(a, f0, rows, seg, c, [&](uint32_t key, int) { gt += key > K ? 1u : 0u; eq += key == K ? 1u : 0u; });
    a.cnt[((int64_t)v * a.nseg + seg) * a.C + c] = make_uint2(gt, eq);
}

// grid (class tiles, V), 1024 threads: lane = class, wave w owns a contiguous sixteenth of the video's segments
__global__ __launch_bounds__(1024) void topa_prefix_kernel(const TopaArgs a)
{
    __shared__ uint32_t sg[16][64], se[16][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int v = blockIdx.y, c = blockIdx.x * 64 + lane;
    int f0, rows;
    topa_range(a, v, f0, rows);
    const int ns = (rows + kTopaRows - 1) / kTopaRows, per = (ns + 15) / 16;
    const int s0 = min(ns, w * per), s1 = min(ns, s0 + per);
    const bool on = c < a.C;
    uint2 *cnt = a.cnt + (int64_t)v * a.nseg * a.C + c;
    uint32_t gt = 0u, eq = 0u;
    if (on)
        for (int s = s0; s < s1; ++s) {
            const uint2 q = cnt[(int64_t)s * a.C];
            gt += q.x; eq += q.y;
        }
    sg[w][lane] = gt; se[w][lane] = eq;
    __syncthreads();
    if (!on) return;
    const uint2 st = a.state[(int64_t)v * a.C + c];
    const uint32_t need = st.x ? st.y : 0u;          // K = 0: the keys "== K" are the non-candidates
    uint32_t gpre = 0u, epre = 0u;
    for (int k = 0; k < w; ++k) { gpre += sg[k][lane]; epre += se[k][lane]; }
    if (w == 0) {
        uint32_t gall = 0u, eall = 0u;
        for (int k = 0; k < 16; ++k) { gall += sg[k][lane]; eall += se[k][lane]; }
        a.nrec[(int64_t)v * a.C + c] = min(gall + min(eall, need), (uint32_t)a.T);
    }
    for (int s = s0; s < s1; ++s) {
        const uint2 q = cnt[(int64_t)s * a.C];
        cnt[(int64_t)s * a.C] = make_uint2(gpre + min(epre, need), epre);
        gpre += q.x; epre += q.y;
    }
}

// grid as topa_count_kernel
__global__ __launch_bounds__(kTopaLT) void topa_gather_kernel(const TopaArgs a)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int v = blockIdx.z, c = blockIdx.y * 64 + lane, seg = blockIdx.x * (kTopaLT / 64) + w;
    int f0, rows;
    topa_range(a, v, f0, rows);
    if (c >= a.C || (int64_t)seg * kTopaRows >= rows) return;
    const uint2 st = a.state[(int64_t)v * a.C + c];
    const uint32_t K = st.x, need = st.x ? st.y : 0u;
    const uint2 q = a.cnt[((int64_t)v * a.nseg + seg) * a.C + c];
    uint32_t pos = q.x, eseen = q.y;
    unsigned long long *rec = a.rec + ((int64_t)v * a.C + c) * a.T;
    topa_walk(a, f0, rows, seg, c, [&](uint32_t key, int r) {
        bool take = key > K;
        if (key == K) { take = eseen < need; ++eseen; }
        if (take) {
            if (pos < (uint32_t)a.T) rec[pos] = ((unsigned long long)key << 32) | (uint32_t)~(uint32_t)r;
            ++pos;
        }
    });
}

// grid (C, V), 256 threads; N = the power of two >= T
__global__ __launch_bounds__(kTopaLT) void topa_emit_kernel(const TopaArgs a, const int N)
{
    __shared__ unsigned long long sk[kTopaMaxT];
    const int tid = threadIdx.x;
    const int c = blockIdx.x, v = blockIdx.y;
    const int64_t vc = (int64_t)v * a.C + c;
    int f0, rows;
    topa_range(a, v, f0, rows);
    const int n = (int)a.nrec[vc];
    for (int i = tid; i < N; i += kTopaLT) sk[i] = i < n ? a.rec[vc * a.T + i] : 0ull;
    for (int k = 2; k <= N; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int i = tid; i < N; i += kTopaLT) {
                const int x = i ^ j;
                if (x > i) {
                    const unsigned long long p = sk[i], q = sk[x];
                    if ((i & k) == 0 ? p < q : p > q) { sk[i] = q; sk[x] = p; }
                }
            }
        }
    __syncthreads();
    for (int t = tid; t < a.T; t += kTopaLT) {
        const int64_t o = (int64_t)v * a.ovs + (int64_t)c * a.ocs + t;
        int32_t fr = 0, bi = -1;
        float4 bx = make_float4(0.f, 0.f, 0.f, 0.f);
        float sc = 0.f;
        const uint32_t r = t < n ? ~(uint32_t)sk[t] : 0xFFFFFFFFu;
        if (r < (uint32_t)rows) {        // (a record always names a row of the video: nothing is read beyond it)
            const int f = (int)(r / (uint32_t)a.B);
            bi = (int32_t)(r - (uint32_t)f * (uint32_t)a.B);
            const int64_t e = (int64_t)(f0 + f) * a.B + bi;
            fr = (a.frame_mode ? f0 + f : f) + 1;
            bx = a.boxes[e];
            sc = a.scores[e * a.C + c];
        }
        a.oframes[o] = fr; a.oindex[o] = bi; a.oboxes[o] = bx; a.oscores[o] = sc;
    }
}

}  // namespace vdet
