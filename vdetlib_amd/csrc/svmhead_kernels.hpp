// The SVM head of the CNN scorers on the device (vdet_svm_head, include/vdet_hip.h): rcnn_scoring / rcnn_sampling_scoring
// (reference vdet/tubelet_cls.py:102-194) after the net -- svm_scores (vdet/image_det.py:109-114) for the ONE class column a
// window needs, the max / argmax over the G = num + 1 windows of a box (:166-189), and the scatter into the [C,T,F] layout.
//
//     s[m] = sum_k (feat[m,k] * scale) * W[k, col_g] + B[col_g]        g = m / G, col_g = cols[slot[g,0]]
//
// in the compute type CT (f64 or f32): feat is converted to CT exactly (f16 / bf16 / f32 / f64 storage), feat * scale is rounded
// once, the product with W is rounded, every addition is rounded; the library is built with -ffp-contract=off, so no two of
// these fuse.  tests/svm_spec.py states the same arithmetic in numpy and the two are compared bit for bit.
//
// THE ACCUMULATION ORDER (independent of N, G, the grid and the feature storage type):
//   1. k is cut into units of 8 consecutive elements; unit u = k / 8 belongs to lane u % 64, in round u / 64.  So lane l owns
//      k = (r*64 + l)*8 + i for r = 0, 1, ... and i = 0..7, as far as k < K.
//   2. A lane adds its products to ONE accumulator that starts at +0, k ascending (r outer, i inner):
//      acc = acc + (feat[k]*scale) * W[k].  A k >= K contributes no operation.
//   3. The 64 accumulators are combined by a butterfly: for d = 32, 16, 8, 4, 2, 1: acc[l] = acc[l] + acc[l ^ d], all lanes at
//      once.  (IEEE addition is commutative, so every lane ends with the same value; lane 0's is used.)
//   4. s = acc + B[col].
//   The argmax over a group follows np.argmax: the first maximum wins, a NaN wins at its first occurrence.
//
// svm_head_kernel<FeatT, CT, NR, VEC>   one WAVE per run of `gpw` consecutive groups, four waves per workgroup, on a 1-D grid.
//     The wave index is made uniform with readfirstlane, so the slot row, the class column and the count are scalar loads and
//     every branch on them is wave-uniform.  NR = 1, 2: K <= NR*512 -- the lane's part of the class column (NR*8 values of the
//     W^T copy, where a column is contiguous) is loaded ONCE per run of groups that share the column and stays in registers
//     while the group's feature rows stream through, up to four rows in flight (kSvmBytesInFlight per lane).  NR = 0: any K, the
//     chunked path -- rounds of 512 k, the column re-read from W^T (L2) per row.  VEC: K % 8 == 0 and 16-byte aligned rows: a
//     unit is read with 16-byte loads (one for 16-bit storage, two for f32, four for f64); otherwise element loads with a
//     bound check per element (NR = 0 only: odd K is no hot shape).  Features are read exactly once.  Window and element
//     offsets are 64-bit.  No atomics on a result path: the one atomicOr latches the error flag, and the count of groups
//     without a window goes through one int per wave and svm_nbad_kernel's sum.
// svm_wt_kernel<WT, CT>   W [K,M] -> W^T [M,K] in CT through a 32 x 33 LDS tile (both sides coalesced).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vdet {

constexpr int kStSvmBad = 2048;         // vdet_svm_head: a slot row outside shape or a class column outside W (the group is skipped)
constexpr int kSvmUnit = 8;             // consecutive k of one lane
constexpr int kSvmRound = 64 * kSvmUnit;
constexpr int kSvmRegRounds = 2;        // the class column stays in registers up to K = kSvmRegRounds * kSvmRound = 1024
constexpr int kSvmBytesInFlight = 256;  // feature bytes a lane requests before it computes (register path)

struct SvmBf16 { uint16_t u; };

struct SvmHeadArgs {
    const void *feat;           // [N*G, K] FeatT
    int64_t N, K, M;
    int G;
    const void *wt;             // [M, K] CT
    const void *bias;           // [M] f64 / f32, or null
    int bias_f64;
    double scale;
    const int32_t *slot;        // [N,3] (c,t,f) or null (c = 0, compact outputs only)
    const int32_t *count;       // [1] or null (N)
    const int32_t *cols;        // [C] or null (identity)
    int64_t C, F;
    int T;
    const double *sboxes;       // [N,G,4] or null
    const uint8_t *ok;          // [N*G] or null
    void *det;                  // [C,T,F] CT or null
    int32_t *arg;               // [C,T,F] or null
    double *tboxes;             // [C,T,F,4] with slot, [N,4] without; or null
    void *score;                // [N] CT
    int32_t *arg_flat;          // [N]
    int32_t *wavebad;           // [waves]
    int gpw;                    // groups per wave
    int64_t nwaves;
    int *status;
};

template <typename CT, typename FeatT> __device__ __forceinline__ CT svm_cvt(FeatT v) { return (CT)v; }
template <> __device__ __forceinline__ float svm_cvt<float, SvmBf16>(SvmBf16 v) { return __uint_as_float((uint32_t)v.u << 16); }
template <> __device__ __forceinline__ double svm_cvt<double, SvmBf16>(SvmBf16 v) { return (double)__uint_as_float((uint32_t)v.u << 16); }

template <typename E> struct alignas(16) SvmPack { E e[16 / sizeof(E)]; };

// the unit that starts at element k0 of a row: 16-byte loads when VEC (then k0 < K means the whole unit is inside), else
// element loads; elements at or behind K are not read
template <typename E, bool VEC> __device__ __forceinline__ void svm_load_unit(const E *row, int64_t k0, int64_t K, E out[kSvmUnit])
{
    if (VEC) {
        constexpr int per = 16 / sizeof(E), packs = kSvmUnit / per;
        if (k0 < K) {
#pragma unroll
            for (int p = 0; p < packs; ++p) {
                const SvmPack<E> v = *reinterpret_cast<const SvmPack<E> *>(row + k0 + p * per);
#pragma unroll
                for (int i = 0; i < per; ++i) out[p * per + i] = v.e[i];
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < kSvmUnit; ++i)
            if (k0 + i < K) out[i] = row[k0 + i];
    }
}

// steps 1 and 2 of the order for one unit: VEC tests the unit, the element form every k
template <typename FeatT, typename CT, bool VEC>
__device__ __forceinline__ CT svm_unit_dot(CT acc, const FeatT f[kSvmUnit], const CT w[kSvmUnit], int64_t k0, int64_t K, CT scale)
{
    if (VEC) {
        if (k0 < K) {
#pragma unroll
            for (int i = 0; i < kSvmUnit; ++i) {
                const CT p = svm_cvt<CT, FeatT>(f[i]) * scale;
                acc = acc + p * w[i];
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < kSvmUnit; ++i)
            if (k0 + i < K) {
                const CT p = svm_cvt<CT, FeatT>(f[i]) * scale;
                acc = acc + p * w[i];
            }
    }
    return acc;
}

// step 3
template <typename CT> __device__ __forceinline__ CT svm_butterfly(CT acc)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc = acc + __shfl_xor(acc, d, 64);
    return acc;
}

// np.argmax's rule over the windows seen so far, as selects: the score and its index move together
template <typename CT> __device__ __forceinline__ void svm_take(CT s, int j, bool &have, CT &best, int &barg)
{
    const bool upd = !have || (best == best && (s > best || s != s));
    best = upd ? s : best;
    barg = upd ? j : barg;
    have = true;
}

template <typename FeatT, typename CT, int NR, bool VEC>
__global__ __launch_bounds__(256) void svm_head_kernel(const SvmHeadArgs a)
{
    constexpr int NRR = NR > 0 ? NR : 1;
    constexpr int RU0 = kSvmBytesInFlight / (NRR * kSvmUnit * (int)sizeof(FeatT));
    constexpr int RU = NR == 0 ? 1 : (RU0 < 1 ? 1 : RU0 > 4 ? 4 : RU0);           // rows in flight
    const int lane = threadIdx.x & 63;
    const int64_t wv = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (wv >= a.nwaves) return;
    const int G = a.G;
    const int64_t K = a.K;
    int64_t n = a.N;
    if (a.count) {
        const int64_t cn = (int64_t)a.count[0];
        n = cn < 0 ? 0 : (cn < n ? cn : n);
    }
    const int64_t g0 = wv * a.gpw;
    const int64_t g1 = (g0 + a.gpw < a.N) ? g0 + a.gpw : a.N;
    const FeatT *feat = static_cast<const FeatT *>(a.feat);
    const CT *wt = static_cast<const CT *>(a.wt);
    CT *score = static_cast<CT *>(a.score);
    const CT scale = (CT)a.scale;
    const CT nan = (CT)__builtin_nan("");
    CT w[NRR][kSvmUnit];
#pragma unroll
    for (int r = 0; r < NRR; ++r)
#pragma unroll
        for (int i = 0; i < kSvmUnit; ++i) w[r][i] = (CT)0;
    int64_t cur = -1;              // the column held in w
    int nb = 0;
    for (int64_t g = g0; g < g1; ++g) {
        int64_t col = -1, idx = g;
        bool valid = g < n;
        if (valid) {
            int c = 0;
            if (a.slot) {
                c = a.slot[g * 3];
                const int t = a.slot[g * 3 + 1], f = a.slot[g * 3 + 2];
                valid = c >= 0 && c < a.C && t >= 0 && t < a.T && f >= 0 && f < a.F;
                idx = ((int64_t)c * a.T + t) * a.F + f;
            }
            if (valid) {
                col = a.cols ? (int64_t)a.cols[c] : (int64_t)c;
                valid = col >= 0 && col < a.M;
            }
            if (!valid && lane == 0) atomicOr(a.status, kStSvmBad);
        }
        if (!valid) {              // behind the count, or refused: nothing but the compact row is written
            if (lane == 0) {
                score[g] = nan;
                a.arg_flat[g] = -1;
            }
            continue;
        }
        const CT *wcol = wt + col * K;
        if (NR > 0 && col != cur) {
#pragma unroll
            for (int r = 0; r < NRR; ++r) svm_load_unit<CT, VEC>(wcol, ((int64_t)r * 64 + lane) * kSvmUnit, K, w[r]);
            cur = col;
        }
        CT bias = (CT)0;
        if (a.bias) bias = a.bias_f64 ? (CT) static_cast<const double *>(a.bias)[col] : (CT) static_cast<const float *>(a.bias)[col];
        bool have = false;
        CT best = nan;
        int barg = -1;
        const int64_t m0 = g * G;
        if (NR > 0) {
            for (int j0 = 0; j0 < G; j0 += RU) {
                FeatT raw[RU][NRR][kSvmUnit];
#pragma unroll
                for (int u = 0; u < RU; ++u)
                    if (j0 + u < G && (!a.ok || a.ok[m0 + j0 + u])) {
                        const FeatT *row = feat + (m0 + j0 + u) * K;
#pragma unroll
                        for (int r = 0; r < NRR; ++r) svm_load_unit<FeatT, VEC>(row, ((int64_t)r * 64 + lane) * kSvmUnit, K, raw[u][r]);
                    }
#pragma unroll
                for (int u = 0; u < RU; ++u)
                    if (j0 + u < G && (!a.ok || a.ok[m0 + j0 + u])) {
                        CT acc = (CT)0;
#pragma unroll
                        for (int r = 0; r < NRR; ++r)
                            acc = svm_unit_dot<FeatT, CT, VEC>(acc, raw[u][r], w[r], ((int64_t)r * 64 + lane) * kSvmUnit, K, scale);
                        const CT s = svm_butterfly(acc) + bias;
                        svm_take(s, j0 + u, have, best, barg);
                    }
            }
        } else {
            const int64_t rounds = (K + kSvmRound - 1) / kSvmRound;
            for (int j = 0; j < G; ++j) {
                if (a.ok && !a.ok[m0 + j]) continue;
                const FeatT *row = feat + (m0 + j) * K;
                CT acc = (CT)0;
#pragma unroll 2
                for (int64_t r = 0; r < rounds; ++r) {
                    const int64_t k0 = (r * 64 + lane) * kSvmUnit;
                    FeatT f[kSvmUnit];
                    CT wr[kSvmUnit];
                    svm_load_unit<FeatT, VEC>(row, k0, K, f);
                    svm_load_unit<CT, VEC>(wcol, k0, K, wr);
                    acc = svm_unit_dot<FeatT, CT, VEC>(acc, f, wr, k0, K, scale);
                }
                const CT s = svm_butterfly(acc) + bias;
                svm_take(s, j, have, best, barg);
            }
        }
        if (!have) ++nb;
        if (lane == 0) {
            score[g] = best;
            a.arg_flat[g] = barg;
            if (a.det) static_cast<CT *>(a.det)[idx] = best;
            if (a.arg) a.arg[idx] = barg;
        }
        if (a.tboxes && a.sboxes && lane < 4)
            a.tboxes[idx * 4 + lane] = have ? a.sboxes[(m0 + barg) * 4 + lane] : (double)__builtin_nan("");
    }
    if (lane == 0) a.wavebad[wv] = nb;
}

// the groups without a window: the sum of the waves' counts, one workgroup of 1024
__global__ __launch_bounds__(1024) void svm_nbad_kernel(const int32_t *wavebad, int64_t nwaves, int32_t *nbad)
{
    __shared__ int wsum[16];
    int s = 0;
    for (int64_t i = threadIdx.x; i < nwaves; i += 1024) s += wavebad[i];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int tot = 0;
        for (int k = 0; k < 16; ++k) tot += wsum[k];
        *nbad = tot;
    }
}

// W [K,M] (WT) -> W^T [M,K] (CT); grid (ceil(M/32), ceil(K/32)), block (32, 8)
template <typename WT, typename CT>
__global__ __launch_bounds__(256) void svm_wt_kernel(const WT *__restrict__ W, int64_t K, int64_t M, CT *__restrict__ out)
{
    __shared__ CT tile[32][33];
    const int64_t m0 = (int64_t)blockIdx.x * 32, k0 = (int64_t)blockIdx.y * 32;
    for (int y = threadIdx.y; y < 32; y += 8) {
        const int64_t k = k0 + y, m = m0 + threadIdx.x;
        if (k < K && m < M) tile[y][threadIdx.x] = (CT)W[k * M + m];
    }
    __syncthreads();
    for (int y = threadIdx.y; y < 32; y += 8) {
        const int64_t m = m0 + y, k = k0 + threadIdx.x;
        if (m < M && k < K) out[m * K + k] = tile[threadIdx.x][y];
    }
}

}  // namespace vdet
