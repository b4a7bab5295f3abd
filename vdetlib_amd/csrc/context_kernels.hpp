// Multi-context suppression: which classes a video's highest-ranked detection scores belong to, and the
// constant taken off every other class's scores.  A T-CNN stage, like motion_kernels.hpp; the reference has no function for it.
//
// RULE (tests/context_spec.py is the numpy form; the device matches it on bits).  Per video: the candidates are the scores
// that are not NaN (and > thr, f32, with a threshold), n their number; k = min(top, n), or max(1, floor(f64 ratio * f64 n))
// clamped to n; thresh the k-th largest candidate (-0.0 == +0.0, +inf when n == 0); hits[c] the candidates of class c that
// are >= thresh -- every tie counts, so no index order, grid shape or run order can show; high[c] = hits[c] >= min_hits.
//
// SHAPE.  The selection is class-blind: a video's scores are one contiguous run of floats, read AS THEY LIE in chunks of
// kCtxChunk elements, a workgroup per chunk, 16-byte loads between a scalar head and tail.  key = score_key(score), 0 for
// a non-candidate (no candidate has a key below 0x007FFFFF, the key of -inf).  A radix select, most significant digit
// first, over the digits 11 | 11 | 10 bits wide finds the key K of rank k: integer histograms (LDS atomics per workgroup,
// integer adds of the non-zero bins to global), so the counts depend on no order.
//   read 1   ctxs_hist_kernel<0>: the histogram of digit 0.  ctxs_select_kernel: n, k, the bin of rank k -- and how many
//            keys lie at or above that bin's lower bound.  If they fit the video's record scratch the video takes path 0.
//   read 2   ctxs_hist_kernel<1>: the histogram of digit 1 among the keys of the chosen bin (every path needs it, so the
//            choice costs no read) and, on path 0, the (key, class) records of every key at or above the bin.  Path 0 is
//            done with the volume: digit 2 and the per-class count of keys >= K come from the records
//            (ctxs_rec_hist_kernel, ctxs_rec_hits_kernel).  The second select knows how many keys lie at or above the
//            22-bit prefix; if THEY fit, path 1, else (an all-equal volume) path 2.
//   read 3   ctxs_hist_kernel<2>, paths 1 and 2: the histogram of digit 2 and, on path 1 (uniform scores: the top bin
//            of 11 bits holds an eighth of them), the records; the per-class count then comes from them.
//   read 4   ctxs_hits_kernel, path 2 only: the per-class count from the volume.
//   Every path is exact, so all give the same bits.  A kernel returns at its first instruction for a video whose path does
//   not need it: the choice is made on the device, the host never waits.
//   ctxs_finish_kernel writes thresh, n and high.
// 32-bit counters: the host refuses a video of 2^32 elements or more.
//
// LDS atomic contention.  Detector scores share a few exponents, so most lanes of a wave hit one bin of digit 0.
// kCtxPeel rounds of "the first lane's digit: one add of its lane count" run before the per-lane atomics; the value is the
// measured best of 0, 1 and 2.
//
// ctxs_suppress_kernel: one read, one write, the same chunks; the video's `high` row in LDS.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nms_kernels.hpp"       // score_key

#ifndef VDET_CTX_PEEL
#define VDET_CTX_PEEL 1
#endif

namespace vdet {

constexpr int kCtxLT = 256;                  // threads of the chunk kernels
constexpr int kCtxChunk = 32768;             // elements of a chunk (128 KiB): tests/context_cases.py restates it
constexpr int kCtxBins = 2048;               // bins of the widest digit
constexpr int kCtxPeel = VDET_CTX_PEEL;
constexpr uint32_t kCtxRecMax = 1u << 21;    // records per video at most (16 MiB) ...
constexpr uint32_t kCtxRecMin = 4096;        // ... at least, and a 64th of the video's elements in between: one record per wave
                                             // load on average; denser, the record bookkeeping sets the pass's time, not the read
constexpr int kCtxLdsRec = 1024;             // records a workgroup collects in LDS before ONE add to the video's cursor
constexpr int kCtxHitsPer = 8192;            // records of a workgroup of ctxs_rec_hits_kernel
constexpr int kCtxLdsClasses = 4096;         // classes whose hits / high flags a workgroup keeps in LDS (the rest: global)

struct CtxVid {
    int64_t e0, ne;              // the video's elements [e0, e0 + ne) of the volume (both multiples of C)
    int64_t rec0;                // its records start here ...
    uint32_t cap;                // ... and there is room for this many (0: the full-read path is forced)
    uint32_t pad;
};

struct CtxState {
    uint32_t prefix;             // digits found so far (at their place in the key); after the last round the key K
    uint32_t rank;               // rank wanted among the keys that share the prefix
    uint32_t n;                  // candidates
    uint32_t path;               // 0: records from read 2; 1: records from read 3; 2: no records, four reads
    uint32_t nrec;               // records written (a cursor during the read that writes them)
    uint32_t empty;              // n == 0
    uint32_t ge;                 // keys in the bins above the chosen one of round 0
    uint32_t pad;
};

struct CtxArgs {
    const float *scores;
    const CtxVid *vids;          // [V], or null: one video, `one`
    CtxVid one;
    int V, C;
    int use_thr;
    float thr;
    double ratio;
    int64_t top;                 // 0: by ratio
    int64_t min_hits;
    uint32_t *hist;              // [V, kCtxBins], zero between the rounds
    CtxState *state;             // [V]
    uint2 *rec;                  // {key, class}
    float *othresh;              // [V]
    int64_t *on;                 // [V]
    int32_t *ohits;              // [V,C], zero at the start
    uint8_t *ohigh;              // [V,C]
};

__device__ __forceinline__ CtxVid ctxs_vid(const CtxArgs &a, int v) { return a.vids ? a.vids[v] : a.one; }

__device__ __forceinline__ uint32_t ctxs_key(const CtxArgs &a, float s)
{
    const bool cand = !(s != s) && (!a.use_thr || s > a.thr);
    return cand ? score_key(s) : 0u;
}

__device__ __forceinline__ float ctxs_unkey(uint32_t k)       // the float of a candidate's key (-0.0 never has one)
{
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

__device__ __forceinline__ int ctxs_shift(int pass) { return pass == 0 ? 21 : pass == 1 ? 10 : 0; }
__device__ __forceinline__ uint32_t ctxs_digit(uint32_t key, int pass) { return pass == 0 ? key >> 21 : pass == 1 ? (key >> 10) & 2047u : key & 1023u; }
// the bits of the digits before `pass`
__device__ __forceinline__ uint32_t ctxs_pmask(int pass) { return pass == 0 ? 0u : pass == 1 ? 0xFFE00000u : 0xFFFFFC00u; }

// The walk every chunk kernel shares: chunk `ch` of a video whose first element is p[0]; fn(score, offset in the chunk) for
// every element of the chunk, four 16-byte loads in flight per lane.  All lanes of a wave call fn together (`on` false: no
// element), so fn may use wave-wide operations.
template <typename Fn>
__device__ __forceinline__ void ctxs_walk(const float *p, int64_t ne, int64_t ch, Fn fn)
{
    const int tid = threadIdx.x;
    const float *q = p + ch * kCtxChunk;
    const int n = (int)min((int64_t)kCtxChunk, ne - ch * kCtxChunk);
    const int head = min(n, (int)((4u - (uint32_t)(((uintptr_t)q >> 2) & 3u)) & 3u));
    fn(tid < head ? q[tid] : 0.f, tid, tid < head);
    const float4 *q4 = reinterpret_cast<const float4 *>(q + head);
    const int n4 = (n - head) >> 2;
    for (int i0 = 0; i0 < n4; i0 += 4 * kCtxLT) {        // (block-uniform bounds)
        float4 s[4];
        bool on[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u * kCtxLT + tid;
            on[u] = i < n4;
            s[u] = on[u] ? q4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int o = head + 4 * (i0 + u * kCtxLT + tid);
            fn(s[u].x, o, on[u]); fn(s[u].y, o + 1, on[u]); fn(s[u].z, o + 2, on[u]); fn(s[u].w, o + 3, on[u]);
        }
    }
    const int t0 = head + 4 * n4, nt = n - t0;           // (< 4)
    fn(tid < nt ? q[t0 + tid] : 0.f, t0 + tid, tid < nt);
}

// one count into an LDS histogram from every lane with `on`: kCtxPeel times the first such lane's bin takes ONE add of
// the number of lanes that share it; what is left adds per lane
__device__ __forceinline__ void ctxs_count(uint32_t *lh, uint32_t bin, bool on)
{
#pragma unroll
    for (int r = 0; r < kCtxPeel; ++r) {
        const unsigned long long act = __ballot(on);
        if (!act) return;                                                    // (wave-uniform)
        const int first = __ffsll((long long)act) - 1;
        const uint32_t b0 = (uint32_t)__shfl((int)bin, first);
        const unsigned long long same = __ballot(on && bin == b0);
        if ((int)(threadIdx.x & 63) == first) atomicAdd(&lh[b0], (uint32_t)__popcll(same));
        on = on && bin != b0;
    }
    if (on) atomicAdd(&lh[bin], 1u);
}

// slots for the lanes of mask m (all of a wave's lanes call it): one add of their number by the first of them
__device__ __forceinline__ uint32_t ctxs_reserve(uint32_t *counter, unsigned long long m)
{
    const int lane = threadIdx.x & 63, first = __ffsll((long long)m) - 1;
    uint32_t base = 0u;
    if (lane == first) base = atomicAdd(counter, (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int)base, first);
    return base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
}

// grid (chunks of the longest video, V).  PASS 0, 1, 2: the histogram of that digit among the keys that share the digits
// found so far; pass 1 also writes the records of path 0, pass 2 those of path 1; passes 1 and 2 skip an empty video, pass 2
// a video on path 0.
template <int PASS>
__global__ __launch_bounds__(kCtxLT) void ctxs_hist_kernel(const CtxArgs a)
{
    __shared__ uint32_t lh[kCtxBins];
    __shared__ uint2 lrec[PASS > 0 ? kCtxLdsRec : 1];    // the chunk's records: the video's cursor takes one add per workgroup
    __shared__ uint32_t lcur, lbase;                     // (a cursor every wave with a record adds to is a queue of its own)
    const int tid = threadIdx.x, v = blockIdx.y;
    const CtxVid d = ctxs_vid(a, v);
    const int64_t ch = blockIdx.x;
    if (ch * kCtxChunk >= d.ne) return;                  // (block-uniform)
    uint32_t prefix = 0u;
    bool records = false;
    if (PASS > 0) {
        const CtxState st = a.state[v];
        if (st.empty || (PASS == 2 && st.path == 0u)) return;
        prefix = st.prefix;
        records = st.path == (uint32_t)(PASS - 1);
    }
    for (int i = tid; i < kCtxBins; i += kCtxLT) lh[i] = 0u;
    if (tid == 0) lcur = 0u;
    __syncthreads();
    const uint32_t pmask = ctxs_pmask(PASS);
    const uint32_t cbase = (uint32_t)((ch * kCtxChunk) % a.C);      // class of the chunk's first element
    uint2 *rec = a.rec + d.rec0;
    uint32_t *cursor = &a.state[v].nrec;
    ctxs_walk(a.scores + d.e0, d.ne, ch, [&](float s, int o, bool on) {
        const uint32_t key = on ? ctxs_key(a, s) : 0u;
        ctxs_count(lh, ctxs_digit(key, PASS), key != 0u && (key & pmask) == prefix);
        if (PASS > 0 && records) {
            const bool take = key >= prefix && key != 0u;           // at or above the chosen bin's lower bound
            const unsigned long long m = __ballot(take);
            if (m) {                                                 // (wave-uniform; rare: the rank is a small share)
                const uint2 r = make_uint2(key, (cbase + (uint32_t)o) % (uint32_t)a.C);
                const uint32_t lpos = ctxs_reserve(&lcur, m);
                if (take && lpos < (uint32_t)kCtxLdsRec) lrec[lpos] = r;
                const unsigned long long m2 = __ballot(take && lpos >= (uint32_t)kCtxLdsRec);
                if (m2) {                                            // a chunk of more records than LDS holds: straight out
                    const uint32_t pos = ctxs_reserve(cursor, m2);
                    if (take && lpos >= (uint32_t)kCtxLdsRec && pos < d.cap) rec[pos] = r;
                }
            }
        }
    });
    __syncthreads();
    uint32_t *gh = a.hist + (int64_t)v * kCtxBins;
    for (int i = tid; i < kCtxBins; i += kCtxLT) {
        const uint32_t h = lh[i];
        if (h) atomicAdd(&gh[i], h);
    }
    if (PASS > 0 && records) {
        const uint32_t nl = min(lcur, (uint32_t)kCtxLdsRec);
        if (tid == 0 && nl) lbase = atomicAdd(cursor, nl);
        __syncthreads();
        for (uint32_t i = tid; i < nl; i += kCtxLT)
            if (lbase + i < d.cap) rec[lbase + i] = lrec[i];
    }
}

// grid (V), 256 threads.  The bin of the round that holds the wanted rank; clears the histogram for the next round.  Round 0
// also finds n and k; rounds 0 and 1 choose the video's path; round 2 leaves the key K in `prefix`.
__global__ __launch_bounds__(256) void ctxs_select_kernel(const CtxArgs a, const int pass)
{
    __shared__ uint32_t part[256];
    __shared__ uint32_t s_n;
    constexpr int kPer = kCtxBins / 256;
    const int tid = threadIdx.x, v = blockIdx.x;
    uint32_t *gh = a.hist + (int64_t)v * kCtxBins;
    CtxState st = a.state[v];
    uint32_t h[kPer], sum = 0u;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        h[j] = gh[tid * kPer + j];
        gh[tid * kPer + j] = 0u;
        sum += h[j];
    }
    part[tid] = sum;
    __syncthreads();
    uint32_t above = 0u;                 // keys of the round in the bins above this thread's
    for (int t = tid + 1; t < 256; ++t) above += part[t];
    if (pass == 0) {
        if (tid == 0) s_n = above + sum;
        __syncthreads();
        const uint32_t n = s_n;
        uint32_t k;
        if (a.top > 0) k = (uint32_t)min(a.top, (int64_t)n);
        else {
            const double x = floor(a.ratio * (double)n);           // (one f64 product: the spec's)
            k = x < 1.0 ? 1u : x >= (double)n ? n : (uint32_t)x;
        }
        st.prefix = 0u; st.rank = k; st.n = n; st.path = 0u; st.nrec = 0u; st.empty = n == 0u ? 1u : 0u;
        st.ge = 0u; st.pad = 0u;
        if (n == 0u) {
            if (tid == 0) { st.prefix = 0xFFFFFFFFu; a.state[v] = st; }    // no key reaches it
            return;
        }
    } else if (st.empty) {
        return;
    }
    // (n >= 1 and 1 <= rank <= the keys of the round: exactly one bin holds the rank)
#pragma unroll
    for (int j = kPer - 1; j >= 0; --j) {
        if (above < st.rank && st.rank <= above + h[j]) {
            st.prefix |= (uint32_t)(tid * kPer + j) << ctxs_shift(pass);
            st.rank -= above;
            const uint32_t cap = ctxs_vid(a, v).cap;
            if (pass == 0) {
                st.ge = above;
                st.path = above + h[j] > cap ? 1u : 0u;             // the records read 2 would write
            } else if (pass == 1 && st.path == 1u) {
                st.path = (uint64_t)st.ge + above + h[j] > cap ? 2u : 1u;      // ... read 3
            }
            a.state[v] = st;
        }
        above += h[j];
    }
}

// path 0, grid (ceil(records of the largest slice / 1024), V): digit 2 among the records that share the first two digits
__global__ __launch_bounds__(kCtxLT) void ctxs_rec_hist_kernel(const CtxArgs a)
{
    __shared__ uint32_t lh[1024];
    const int tid = threadIdx.x, v = blockIdx.y;
    const CtxState st = a.state[v];
    if (st.empty || st.path != 0u) return;
    const uint32_t r0 = blockIdx.x * 1024u;
    if (r0 >= st.nrec) return;
    for (int i = tid; i < 1024; i += kCtxLT) lh[i] = 0u;
    __syncthreads();
    const uint2 *rec = a.rec + ctxs_vid(a, v).rec0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const uint32_t r = r0 + u * kCtxLT + tid;
        const uint32_t key = r < st.nrec ? rec[r].x : 0u;
        ctxs_count(lh, key & 1023u, key != 0u && (key & 0xFFFFFC00u) == st.prefix);
    }
    __syncthreads();
    uint32_t *gh = a.hist + (int64_t)v * kCtxBins;
    for (int i = tid; i < 1024; i += kCtxLT) {
        const uint32_t h = lh[i];
        if (h) atomicAdd(&gh[i], h);
    }
}

// paths 0 and 1, grid (ceil(records of the largest slice / kCtxHitsPer), V): hits[c] += records of class c with key >= K,
// the classes below kCtxLdsClasses through LDS
__global__ __launch_bounds__(kCtxLT) void ctxs_rec_hits_kernel(const CtxArgs a)
{
    __shared__ uint32_t lc[kCtxLdsClasses];
    const int tid = threadIdx.x, v = blockIdx.y;
    const CtxState st = a.state[v];
    if (st.empty || st.path == 2u) return;
    const uint32_t r0 = blockIdx.x * (uint32_t)kCtxHitsPer, r1 = min(st.nrec, r0 + (uint32_t)kCtxHitsPer);
    if (r0 >= st.nrec) return;
    const int nl = min(a.C, kCtxLdsClasses);
    for (int i = tid; i < nl; i += kCtxLT) lc[i] = 0u;
    __syncthreads();
    const uint2 *rec = a.rec + ctxs_vid(a, v).rec0;
    int32_t *hits = a.ohits + (int64_t)v * a.C;
    for (uint32_t i = r0 + tid; i < r1; i += kCtxLT) {
        const uint2 q = rec[i];
        if (q.x >= st.prefix) {
            if (q.y < (uint32_t)kCtxLdsClasses) atomicAdd(&lc[q.y], 1u);
            else atomicAdd(&hits[q.y], 1);
        }
    }
    __syncthreads();
    for (int i = tid; i < nl; i += kCtxLT) {
        const uint32_t h = lc[i];
        if (h) atomicAdd(&hits[i], (int32_t)h);
    }
}

// path 2, grid as ctxs_hist_kernel: the same count from the volume, the classes below kCtxLdsClasses through LDS
__global__ __launch_bounds__(kCtxLT) void ctxs_hits_kernel(const CtxArgs a)
{
    __shared__ uint32_t lc[kCtxLdsClasses];
    const int tid = threadIdx.x, v = blockIdx.y;
    const CtxVid d = ctxs_vid(a, v);
    const int64_t ch = blockIdx.x;
    if (ch * kCtxChunk >= d.ne) return;
    const CtxState st = a.state[v];
    if (st.empty || st.path != 2u) return;
    const int nl = min(a.C, kCtxLdsClasses);
    for (int i = tid; i < nl; i += kCtxLT) lc[i] = 0u;
    __syncthreads();
    const uint32_t K = st.prefix;
    const uint32_t cbase = (uint32_t)((ch * kCtxChunk) % a.C);
    int32_t *hits = a.ohits + (int64_t)v * a.C;
    ctxs_walk(a.scores + d.e0, d.ne, ch, [&](float s, int o, bool on) {
        const uint32_t key = on ? ctxs_key(a, s) : 0u;
        if (key >= K && key != 0u) {
            const uint32_t c = (cbase + (uint32_t)o) % (uint32_t)a.C;
            if (c < (uint32_t)kCtxLdsClasses) atomicAdd(&lc[c], 1u);
            else atomicAdd(&hits[c], 1);
        }
    });
    __syncthreads();
    for (int i = tid; i < nl; i += kCtxLT) {
        const uint32_t h = lc[i];
        if (h) atomicAdd(&hits[i], (int32_t)h);
    }
}

// grid (ceil(C / 256), V)
__global__ __launch_bounds__(256) void ctxs_finish_kernel(const CtxArgs a)
{
    const int v = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
    const CtxState st = a.state[v];
    if (c == 0) {
        a.othresh[v] = st.empty ? __uint_as_float(0x7F800000u) : ctxs_unkey(st.prefix);
        a.on[v] = (int64_t)st.n;
    }
    if (c < a.C) a.ohigh[(int64_t)v * a.C + c] = (int64_t)a.ohits[(int64_t)v * a.C + c] >= a.min_hits ? 1 : 0;
}

struct CtxSuppressArgs {
    const float *in;
    float *out;
    const uint8_t *high;         // [V,C]
    const CtxVid *vids;
    CtxVid one;
    int C;
    float penalty;
};

// grid (chunks of the longest video, V): out = in - penalty where the class is not high and the score is not NaN; every other
// element is copied.  in == out is allowed: a lane writes only what it has read.
__global__ __launch_bounds__(kCtxLT) void ctxs_suppress_kernel(const CtxSuppressArgs a)
{
    __shared__ uint8_t lhigh[kCtxLdsClasses];
    const int tid = threadIdx.x, v = blockIdx.y;
    const CtxVid d = a.vids ? a.vids[v] : a.one;
    const int64_t ch = blockIdx.x;
    if (ch * kCtxChunk >= d.ne) return;
    const uint8_t *high = a.high + (int64_t)v * a.C;
    const int nl = min(a.C, kCtxLdsClasses);
    for (int i = tid; i < nl; i += kCtxLT) lhigh[i] = high[i];
    __syncthreads();
    const uint32_t C = (uint32_t)a.C;
    const float pen = a.penalty;
    auto one = [&](float s, uint32_t c) {
        const bool hi = (c < (uint32_t)kCtxLdsClasses ? lhigh[c] : high[c]) != 0;
        return (hi || s != s) ? s : s - pen;
    };
    const int64_t e = d.e0 + ch * kCtxChunk;
    const float *q = a.in + e;
    float *w = a.out + e;
    const int n = (int)min((int64_t)kCtxChunk, d.ne - ch * kCtxChunk);
    const uint32_t cbase = (uint32_t)((ch * kCtxChunk) % a.C);
    if ((((uintptr_t)q ^ (uintptr_t)w) & 15u) != 0) {       // the two do not share an alignment: element by element
        uint32_t c = (cbase + (uint32_t)tid) % C;
        const uint32_t step = (uint32_t)kCtxLT % C;
        for (int i = tid; i < n; i += kCtxLT) {
            w[i] = one(q[i], c);
            c += step; if (c >= C) c -= C;
        }
        return;
    }
    const int head = min(n, (int)((4u - (uint32_t)(((uintptr_t)q >> 2) & 3u)) & 3u));
    if (tid < head) w[tid] = one(q[tid], (cbase + (uint32_t)tid) % C);
    const float4 *q4 = reinterpret_cast<const float4 *>(q + head);
    float4 *w4 = reinterpret_cast<float4 *>(w + head);
    const int n4 = (n - head) >> 2;
    uint32_t c = (cbase + (uint32_t)(head + 4 * tid)) % C;
    const uint32_t step = (uint32_t)(4 * kCtxLT) % C;
    auto next = [&](uint32_t x) { return x + 1u == C ? 0u : x + 1u; };
    for (int i0 = 0; i0 < n4; i0 += 4 * kCtxLT) {
        float4 s[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u * kCtxLT + tid;
            s[u] = i < n4 ? q4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u * kCtxLT + tid;
            const uint32_t c1 = next(c), c2 = next(c1), c3 = next(c2);
            const float4 r = make_float4(one(s[u].x, c), one(s[u].y, c1), one(s[u].z, c2), one(s[u].w, c3));
            if (i < n4) w4[i] = r;
            c += step; if (c >= C) c -= C;
        }
    }
    const int t0 = head + 4 * n4;
    if (tid < n - t0) w[t0 + tid] = one(q[t0 + tid], (cbase + (uint32_t)(t0 + tid)) % C);
}

}  // namespace vdet
