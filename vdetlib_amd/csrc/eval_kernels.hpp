// Device evaluator (vdetlib_amd/eval.py on the GPU): greedy true/false-positive matching of detections against the
// ground truth of their (video, frame, class), compaction into a (class, score, tp) stream, and per-class average
// precision over a stable device-wide sort of that stream.  f64 throughout, built with -ffp-contract=off: the operation
// order of eval.py's _iou_1n / average_precision is the specification.  No float atomics on any result path.
#pragma once

namespace vdet {

constexpr int kStEvalList = 64;     // a keep list with a NaN score, an increasing score or an index / count out of range
constexpr int kEvalMaxT = 1024;     // candidates of one (frame, class) group of the tubelet form (= max_tracks)
constexpr int kEvalMaxGt = 256;     // ground-truth boxes of one (video, frame, class)
constexpr int kEvalTile = 4096;     // items per workgroup of the compaction and radix kernels (256 threads x 16)

// numpy's np.maximum / np.minimum: a NaN in either operand propagates
__device__ __forceinline__ double ev_npmax(double a, double b) { return (a != a || b != b) ? __builtin_nan("") : (a > b ? a : b); }
__device__ __forceinline__ double ev_npmin(double a, double b) { return (a != a || b != b) ? __builtin_nan("") : (a < b ? a : b); }

// The ground-truth CSR (vdet_eval_gt_upload): boxes of (video vi, frame, class slot s) are
// boxes[off[vmeta[2vi] + frame * K + s] .. off[... + 1]) for frame < vmeta[2vi + 1].
struct EvGt {
    const double *boxes;
    const int32_t *off;
    const int64_t *vmeta;
    int K;
    int rule;          // 0 VOC, 1 ILSVRC
    double thr;
};

__device__ __forceinline__ void ev_gt_range(const EvGt &g, int vi, int64_t frame1, int slot, int &g0, int &ng)
{
    g0 = 0;
    ng = 0;
    if (vi < 0 || slot < 0) return;
    const int64_t base = g.vmeta[2 * vi], nf = g.vmeta[2 * vi + 1];
    if (frame1 < 0 || frame1 >= nf) return;
    const int64_t o = base + frame1 * g.K + slot;
    g0 = g.off[o];
    ng = g.off[o + 1] - g0;
}

// np.argmax order for the VOC rule: NaN is the maximum, the first of equal values wins
__device__ __forceinline__ bool ev_voc_better(double a, int ja, double b, int jb)
{
    const bool an = a != a, bn = b != b;
    if (an || bn) return an && (!bn || ja < jb);
    if (a != b) return a > b;
    return ja < jb;
}

// One detection against the group's ground truths (one wave, lanes over the ground truths).  Returns the index of the
// ground truth it matches (the caller marks it used), or -1 for a false positive.  Wave-uniform result.
__device__ int ev_match_one(const EvGt &g, int g0, int ng, double b0, double b1, double b2, double b3, const uint8_t *used)
{
    const int lane = threadIdx.x & 63;
    const double a = (b2 - b0 + 1.0) * (b3 - b1 + 1.0);
    double best = -__builtin_inf();
    int bj = 0x7FFFFFFF;
    for (int j = lane; j < ng; j += 64) {
        const double *q = g.boxes + (int64_t)(g0 + j) * 4;
        const double q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
        const double ix1 = ev_npmax(b0, q0), iy1 = ev_npmax(b1, q1);
        const double ix2 = ev_npmin(b2, q2), iy2 = ev_npmin(b3, q3);
        const double iw = ev_npmax(0.0, ix2 - ix1 + 1.0), ih = ev_npmax(0.0, iy2 - iy1 + 1.0);
        const double inter = iw * ih;
        const double b = (q2 - q0 + 1.0) * (q3 - q1 + 1.0);
        double ov = inter / (a + b - inter);
        if (g.rule == 0) {
            if (used[j]) ov = -1.0;
            if (ev_voc_better(ov, j, best, bj)) { best = ov; bj = j; }
        } else if (!used[j]) {
            const double w = q2 - q0 + 1.0, h = q3 - q1 + 1.0;
            const double tj = ev_npmin(g.thr, (w * h) / ((w + 10.0) * (h + 10.0)));
            if (iw > 0.0 && ih > 0.0 && ov >= tj && ov > best) { best = ov; bj = j; }
        }
    }
    for (int m = 1; m < 64; m <<= 1) {
        const double ob = __shfl_xor(best, m);
        const int oj = __shfl_xor(bj, m);
        const bool take = g.rule == 0 ? ev_voc_better(ob, oj, best, bj) : (ob > best || (ob == best && oj < bj));
        if (take) { best = ob; bj = oj; }
    }
    if (bj >= ng) return -1;
    if (g.rule == 0) return best >= g.thr ? bj : -1;
    return best > -__builtin_inf() ? bj : -1;
}

// Tubelet form, V videos in one launch: grid (sum_v F_v, C), one wave per (frame, class) group.  Video v's arrays start
// at element C*T*foff[v] and are [C,T,F_v] (boxes: stride `bstride` floats per element, the first 4 are the box).
// Writes the dense per-element result: dtp -1 (no detection) / 0 (fp) / 1 (tp), dsc the f64 score, dslot the class slot.
__global__ __launch_bounds__(64) void eval_match_tracks_kernel(EvGt g, const int64_t *foff, int V, const int32_t *vid, int C, int T,
                                                               const float *boxes, int bstride, const double *sc64,
                                                               const float *sc32, const int32_t *ntracks, const int32_t *col_slot,
                                                               int8_t *dtp, double *dsc, int32_t *dslot)
{
    __shared__ double s_sc[kEvalMaxT];
    __shared__ int s_t[kEvalMaxT];
    __shared__ int s_ord[kEvalMaxT];
    __shared__ uint8_t s_used[kEvalMaxGt];
    const int lane = threadIdx.x;
    const int64_t fg = blockIdx.x;
    const int c = blockIdx.y;
    int lo = 0, hi = V;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (foff[mid] <= fg) lo = mid; else hi = mid;
    }
    const int v = lo;
    const int64_t f0 = foff[v], Fv = foff[v + 1] - f0, f = fg - f0;
    const int slot = col_slot[c];
    int ntr = ntracks[(int64_t)v * C + c];
    ntr = ntr < 0 ? 0 : (ntr > T ? T : ntr);
    const int64_t base = (int64_t)C * T * f0;
    for (int t = lane; t < T; t += 64) {
        const int64_t idx = base + ((int64_t)c * T + t) * Fv + f;
        const double s = sc64 ? sc64[idx] : (double)sc32[idx];
        const bool valid = slot >= 0 && t < ntr && !(s != s);
        dtp[idx] = valid ? 0 : -1;
        dsc[idx] = s;
        dslot[idx] = slot;
    }
    int g0, ng;
    ev_gt_range(g, vid[v], f + 1, slot, g0, ng);
    if (ng <= 0 || ng > kEvalMaxGt) return;
    // the group's candidates, in t order
    int n = 0;
    for (int t0 = 0; t0 < ntr; t0 += 64) {
        const int t = t0 + lane;
        double s = 0.0;
        bool valid = false;
        if (t < ntr) {
            const int64_t idx = base + ((int64_t)c * T + t) * Fv + f;
            s = sc64 ? sc64[idx] : (double)sc32[idx];
            valid = !(s != s);
        }
        const unsigned long long m = __ballot(valid);
        if (valid) {
            const int pos = n + __popcll(m & ((1ull << lane) - 1ull));
            s_sc[pos] = s;
            s_t[pos] = t;
        }
        n += __popcll(m);
    }
    for (int j = lane; j < ng; j += 64) s_used[j] = 0;
    __syncthreads();
    // descending score, ties by ascending t (Python's stable sorted() over the (t, f) input order)
    for (int i = lane; i < n; i += 64) {
        const double si = s_sc[i];
        int r = 0;
        for (int j = 0; j < n; ++j) {
            const double sj = s_sc[j];
            r += (sj > si || (sj == si && j < i)) ? 1 : 0;
        }
        s_ord[r] = i;
    }
    __syncthreads();
    for (int r = 0; r < n; ++r) {
        const int t = s_t[s_ord[r]];
        const int64_t idx = base + ((int64_t)c * T + t) * Fv + f;
        const float *bp = boxes + idx * bstride;
        const int j = ev_match_one(g, g0, ng, (double)bp[0], (double)bp[1], (double)bp[2], (double)bp[3], s_used);
        __syncthreads();
        if (j >= 0 && lane == 0) {
            s_used[j] = 1;
            dtp[idx] = 1;
        }
        __syncthreads();
    }
}

// Keep-list form: grid (F, C), one wave per (frame, class) list; dense results at ((f*C + c)*cap + k).  The list is walked
// in its own order, which must be non-increasing in score (else kStEvalList is latched; nothing is re-sorted).
__global__ __launch_bounds__(64) void eval_match_keep_kernel(EvGt g, int vi, int C, int B, int layout, const float *boxes,
                                                             const float *scores, const int32_t *keep_idx, const int32_t *keep_cnt,
                                                             int64_t cap, const int32_t *col_slot, int8_t *dtp, double *dsc,
                                                             int32_t *dslot, int *status)
{
    __shared__ uint8_t s_used[kEvalMaxGt];
    const int lane = threadIdx.x;
    const int64_t f = blockIdx.x;
    const int c = blockIdx.y;
    const int slot = col_slot[c];
    int n = keep_cnt[f * C + c];
    bool bad = false;
    if (n < 0 || n > cap) {
        bad = true;
        n = n < 0 ? 0 : (int)cap;
    }
    const int64_t row = (f * C + c) * cap;
    auto score_of = [&](int b) -> double {
        return (double)(layout == 0 ? scores[(f * B + b) * C + c] : scores[(f * C + c) * B + b]);
    };
    for (int64_t k = lane; k < cap; k += 64) {
        bool valid = false;
        double s = __builtin_nan("");
        if (k < n) {
            const int b = keep_idx[row + k];
            if (b < 0 || b >= B) {
                bad = true;
            } else {
                s = score_of(b);
                if (s != s) bad = true; else valid = true;
                if (k > 0) {
                    const int bp = keep_idx[row + k - 1];
                    if (bp >= 0 && bp < B && s > score_of(bp)) bad = true;
                }
            }
        }
        dtp[row + k] = (valid && slot >= 0) ? 0 : -1;
        dsc[row + k] = s;
        dslot[row + k] = slot;
    }
    if (__ballot(bad) != 0ull) {
        if (lane == 0) atomicOr(status, kStEvalList);
        return;
    }
    int g0, ng;
    ev_gt_range(g, vi, f + 1, slot, g0, ng);
    if (ng <= 0 || ng > kEvalMaxGt) return;
    for (int j = lane; j < ng; j += 64) s_used[j] = 0;
    __syncthreads();
    for (int k = 0; k < n; ++k) {
        const int b = keep_idx[row + k];
        const float *bp = boxes + ((int64_t)f * B + b) * 4;
        const int j = ev_match_one(g, g0, ng, (double)bp[0], (double)bp[1], (double)bp[2], (double)bp[3], s_used);
        __syncthreads();
        if (j >= 0 && lane == 0) {
            s_used[j] = 1;
            dtp[row + k] = 1;
        }
        __syncthreads();
    }
}

// ---- order-preserving compaction of the dense results into the stream -------------------------------------------------

__device__ __forceinline__ int64_t ev_block_sum_256(int64_t v, int64_t *s_red)
{
    const int tid = threadIdx.x;
    s_red[tid] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) s_red[tid] += s_red[tid + o];
        __syncthreads();
    }
    const int64_t r = s_red[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(256) void eval_count_kernel(const int8_t *dtp, int64_t N, int64_t *bcnt)
{
    __shared__ int64_t s_red[256];
    const int64_t tile = (int64_t)blockIdx.x * kEvalTile;
    int64_t cnt = 0;
    for (int r = 0; r < kEvalTile / 256; ++r) {
        const int64_t i = tile + r * 256 + threadIdx.x;
        if (i < N && dtp[i] >= 0) ++cnt;
    }
    cnt = ev_block_sum_256(cnt, s_red);
    if (threadIdx.x == 0) bcnt[blockIdx.x] = cnt;
}

// exclusive scan of n values in one workgroup of 1024 threads (contiguous chunks per thread); *total = the sum
template <typename T>
__global__ __launch_bounds__(1024) void eval_scan_kernel(const T *in, int64_t n, T *out, T *total)
{
    __shared__ T s[1024];
    const int tid = threadIdx.x;
    const int64_t chunk = (n + 1023) / 1024;
    const int64_t b = tid * chunk, e = b + chunk < n ? b + chunk : n;
    T sum = 0;
    for (int64_t i = b; i < e; ++i) sum += in[i];
    s[tid] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const T v = tid >= o ? s[tid - o] : (T)0;
        __syncthreads();
        s[tid] += v;
        __syncthreads();
    }
    T run = s[tid] - sum;
    for (int64_t i = b; i < e; ++i) {
        const T x = in[i];
        out[i] = run;
        run += x;
    }
    if (tid == 1023 && total) *total = s[1023];
}

__global__ __launch_bounds__(256) void eval_scatter_kernel(const int8_t *dtp, const double *dsc, const int32_t *dslot, int64_t N,
                                                           const int64_t *boff, int64_t st_len, int32_t *st_slot, double *st_sc,
                                                           uint8_t *st_tp)
{
    __shared__ int s_w[4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t tile = (int64_t)blockIdx.x * kEvalTile;
    int64_t run = st_len + boff[blockIdx.x];
    for (int r = 0; r < kEvalTile / 256; ++r) {
        const int64_t i = tile + r * 256 + tid;
        const int8_t t = i < N ? dtp[i] : (int8_t)-1;
        const bool v = t >= 0;
        const unsigned long long m = __ballot(v);
        if (lane == 0) s_w[w] = __popcll(m);
        __syncthreads();
        int before = 0, all = 0;
        for (int k = 0; k < 4; ++k) {
            before += k < w ? s_w[k] : 0;
            all += s_w[k];
        }
        if (v) {
            const int64_t p = run + before + __popcll(m & ((1ull << lane) - 1ull));
            st_slot[p] = dslot[i];
            st_sc[p] = dsc[i];
            st_tp[p] = (uint8_t)t;
        }
        run += all;
        __syncthreads();
    }
}

// ---- stable LSD radix sort of the stream by (class slot asc, score desc) ------------------------------------------------
// key: the f64 score (-0.0 -> +0.0) mapped to a u64 that orders descending scores ascending; val: slot << 32 | position.
// Passes 0..7 sort the key bytes, passes 8.. the slot bytes (val bits 32..).

__global__ __launch_bounds__(256) void eval_key_kernel(const int32_t *slot, const double *sc, int64_t n, uint64_t *key, uint64_t *val)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double s = sc[i];
    if (s == 0.0) s = 0.0;
    const uint64_t bits = (uint64_t)__double_as_longlong(s);
    const uint64_t asc = (bits >> 63) ? ~bits : (bits | 0x8000000000000000ull);
    key[i] = ~asc;
    val[i] = ((uint64_t)(uint32_t)slot[i] << 32) | (uint64_t)(uint32_t)i;
}

__device__ __forceinline__ uint32_t ev_digit(uint64_t k, uint64_t v, int pass)
{
    return pass < 8 ? (uint32_t)(k >> (8 * pass)) & 255u : (uint32_t)(v >> (32 + 8 * (pass - 8))) & 255u;
}

__global__ __launch_bounds__(256) void eval_hist_kernel(const uint64_t *key, const uint64_t *val, int64_t n, int pass, uint32_t *hist)
{
    __shared__ uint32_t h[256];
    const int tid = threadIdx.x;
    h[tid] = 0;
    __syncthreads();
    const int64_t tile = (int64_t)blockIdx.x * kEvalTile;
    for (int r = 0; r < kEvalTile / 256; ++r) {
        const int64_t i = tile + r * 256 + tid;
        if (i < n) atomicAdd(&h[ev_digit(key[i], val[i], pass)], 1u);
    }
    __syncthreads();
    hist[(int64_t)tid * gridDim.x + blockIdx.x] = h[tid];
}

__global__ __launch_bounds__(256) void eval_radix_scatter_kernel(const uint64_t *kin, const uint64_t *vin, int64_t n, int pass,
                                                                 const uint32_t *off, uint64_t *kout, uint64_t *vout)
{
    __shared__ uint32_t s_base[256];
    __shared__ uint32_t s_wc[4][256];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    s_base[tid] = off[(int64_t)tid * gridDim.x + blockIdx.x];
    const int64_t tile = (int64_t)blockIdx.x * kEvalTile;
    for (int r = 0; r < kEvalTile / 256; ++r) {
        for (int k = 0; k < 4; ++k) s_wc[k][tid] = 0;
        __syncthreads();
        const int64_t i = tile + r * 256 + tid;
        const bool valid = i < n;
        uint64_t k = 0, v = 0;
        uint32_t d = 0;
        if (valid) {
            k = kin[i];
            v = vin[i];
            d = ev_digit(k, v, pass);
        }
        unsigned long long match = __ballot(valid);
        for (int bit = 0; bit < 8; ++bit) {
            const bool on = (d >> bit) & 1u;
            const unsigned long long bm = __ballot(valid && on);
            match &= on ? bm : ~bm;
        }
        const int rank = __popcll(match & ((1ull << lane) - 1ull));
        if (valid && rank == 0) s_wc[w][d] = (uint32_t)__popcll(match);
        __syncthreads();
        if (valid) {
            uint32_t p = s_base[d] + rank;
            for (int q = 0; q < w; ++q) p += s_wc[q][d];
            kout[p] = k;
            vout[p] = v;
        }
        __syncthreads();
        s_base[tid] += s_wc[0][tid] + s_wc[1][tid] + s_wc[2][tid] + s_wc[3][tid];
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void eval_perm_kernel(const uint64_t *val, int64_t n, int32_t *perm)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) perm[i] = (int32_t)(uint32_t)val[i];
}

// ---- per-class AP (eval.py: average_precision) ----------------------------------------------------------------------
// One workgroup per class slot over its segment of the sorted stream, walked in 256-entry chunks from the END: the
// precision envelope is a suffix maximum, and ctp at a position is the class total minus the tps behind it.
__global__ __launch_bounds__(256) void eval_ap_kernel(const uint64_t *val, const uint8_t *tp, int64_t n, const int64_t *ngt, double *ap)
{
    __shared__ int64_t s_seg[2];
    __shared__ int64_t s_red[256];
    __shared__ int s_i[256];
    __shared__ double s_d[256];
    const int tid = threadIdx.x;
    const uint32_t k = blockIdx.x;
    if (tid < 2) {
        const uint32_t want = k + (uint32_t)tid;          // lower bound of slot k (tid 0) and k + 1 (tid 1)
        int64_t lo = 0, hi = n;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if ((uint32_t)(val[mid] >> 32) < want) lo = mid + 1; else hi = mid;
        }
        s_seg[tid] = lo;
    }
    __syncthreads();
    const int64_t lo = s_seg[0], len = s_seg[1] - s_seg[0];
    const int64_t ng = ngt[k];
    if (ng <= 0) {
        if (tid == 0) ap[k] = __builtin_nan("");
        return;
    }
    int64_t cnt = 0;
    for (int64_t p = tid; p < len; p += 256) cnt += tp[(uint32_t)val[lo + p]] ? 1 : 0;
    const int64_t total = ev_block_sum_256(cnt, s_red);
    const double dng = (double)ng;
    int64_t after = 0;          // tps behind the current chunk
    double env = 0.0;           // precision envelope behind the current chunk (mpre's trailing 0)
    double acc = 0.0;
    for (int64_t ch = (len + 255) / 256 - 1; ch >= 0; --ch) {
        const int64_t p = ch * 256 + tid;
        const bool valid = p < len;
        const int t = valid ? (tp[(uint32_t)val[lo + p]] ? 1 : 0) : 0;
        s_i[tid] = t;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {           // inclusive suffix sum
            const int x = tid + o < 256 ? s_i[tid + o] : 0;
            __syncthreads();
            s_i[tid] += x;
            __syncthreads();
        }
        const int64_t ctp = total - after - (s_i[tid] - t);
        const double prec = valid ? (double)ctp / (double)(p + 1) : 0.0;
        s_d[tid] = prec;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {           // inclusive suffix max
            const double x = tid + o < 256 ? s_d[tid + o] : 0.0;
            __syncthreads();
            if (x > s_d[tid]) s_d[tid] = x;
            __syncthreads();
        }
        const double e = s_d[tid] > env ? s_d[tid] : env;
        if (valid && t) acc += ((double)ctp / dng - (double)(ctp - 1) / dng) * e;
        const int chunk_tp = s_i[0];
        const double chunk_max = s_d[0];
        __syncthreads();
        after += chunk_tp;
        if (chunk_max > env) env = chunk_max;
    }
    // fixed-order reduction of the per-thread sums
    s_d[tid] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) s_d[tid] = s_d[tid] + s_d[tid + o];
        __syncthreads();
    }
    if (tid == 0) ap[k] = s_d[0];
}

}  // namespace vdet
