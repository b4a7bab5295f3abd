// Device form of the tubelet temporal-convolution scorer (score_conv_cls, reference vdet/tubelet_cls.py:15-51, with the build's
// own network of vdetlib_amd/vdet/tcn.py): channel assembly from the device tracks, the whole network in ONE launch, and the
// ground-truth overlap channel (tubelets_overlap, reference utils/protocol.py:467-489) over the evaluator's table.
//
// Tubelet (c, t) of a video = the frames of tracks[c, t] whose row is not NaN (column 0, as ops.tracks_to_proto tests it), in
// frame order, compacted to a series of length L; t >= ntracks[c] does not exist.  Video v of a batch starts at element
// C*T*foff[v] of every [C,T,F_v] array (vdet_video_batch's layout).
//
// Arithmetic of the network = conv1d_kernel's and softmax_channels_kernel's (tubelet_kernels.hpp), element for element:
// acc = b[co]; for ci, for k: acc = acc + w * x in f32, no contraction (the library is built with -ffp-contract=off), "same"
// zero padding at the ends of the COMPACTED series, ReLU between layers, channel softmax at the end.  Results are therefore
// bit-identical to the per-tubelet path whatever the tiling below.
#pragma once

#include "temporal_kernels.hpp"   // iou_f64_pair
#include "eval_kernels.hpp"       // EvGt, ev_gt_range

namespace vdet {

constexpr int kTcnMaxLayers = 16;       // layers of one net
constexpr int kTcnMaxChannels = 4096;   // channels of any layer (inputs included)
constexpr int kTcnMaxK = 31;            // taps per layer (odd), like vdet_temporal_conv_f32
constexpr int kTcnLdsBudget = 48 * 1024;   // activations of one workgroup: three workgroups share a CU's 160 KiB
constexpr int kTcnMinTile = 16;         // a series is not tiled into pieces shorter than this (or than the halo)
constexpr int kTcnThreads = 256;

// channel codes of the assembly (the blob names of vdet/tubelet_cls.py::_tcn_channels)
enum { kChDet = 0, kChTrack = 1, kChAnchor = 2, kChAbsAnchor = 3, kChGtOverlap = 4, kChLabel = 5, kChCount = 6 };

struct TcnLayer {
    int cin, cout, k;
    int woff, boff;      // float offsets of W [cout, cin, k] and b [cout] in the packed parameter block
    int rem;             // halo the LATER layers still need on each side of this layer's output
};

struct TcnNet {
    TcnLayer l[kTcnMaxLayers];
    int n;               // layers
    int cin;             // input channels
    int maxc;            // widest activation (inputs included)
    int halo;            // receptive radius of the whole net: sum of k/2
};

struct TcnChannels {
    int n;
    int code[16];
};

// ------------------------------------------------------------------------------------------------
// Channel assembly: grid (C*T, V), one wave per tubelet slot.  Writes, at the slot's base b = C*T*f0 + (c*T + t)*F_v:
//   frames[b + j]        frame (0-based) of the j-th box,
//   x[b*Cin + q*L + j]   channel q of the j-th box (channel-major, compact),
//   tub_base / tub_len   the slot's base and L (0: no tubelet),
//   conv_out[b + f]      NaN for every frame (the network kernel then overwrites the frames that have a box).
// Rounding = np.asarray(python floats, dtype='float32'): one round-to-nearest from f64.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void tcn_assemble_kernel(const float *__restrict__ tracks, const int32_t *__restrict__ ntracks,
                                                          const float *__restrict__ anchors, const double *__restrict__ det64,
                                                          const float *__restrict__ det32, const double *__restrict__ gt_overlap,
                                                          const int64_t *__restrict__ foff, int64_t F1, int C, int T, TcnChannels ch,
                                                          float *__restrict__ x, int32_t *__restrict__ frames,
                                                          int64_t *__restrict__ tub_base, int32_t *__restrict__ tub_len,
                                                          float *__restrict__ conv_out)
{
    const int lane = threadIdx.x;
    const int v = blockIdx.y;
    const int ct = blockIdx.x, c = ct / T, t = ct - c * T;
    const int64_t f0 = foff ? foff[v] : 0, Fv = foff ? foff[v + 1] - f0 : F1;
    const int64_t base = (int64_t)C * T * f0 + (int64_t)ct * Fv;
    const int64_t tub = (int64_t)v * C * T + ct;
    const float qnan = __builtin_nanf("");
    int nt = ntracks[(int64_t)v * C + c];
    nt = nt < 0 ? 0 : (nt > T ? T : nt);
    int L = 0;
    for (int64_t fb = 0; fb < Fv; fb += 64) {
        const int64_t f = fb + lane;
        bool has = false;
        if (f < Fv) {
            conv_out[base + f] = qnan;
            const float r0 = tracks[(base + f) * 5];
            has = t < nt && !(r0 != r0);
        }
        L += __popcll(__ballot(has));
    }
    if (lane == 0) {
        tub_base[tub] = base;
        tub_len[tub] = L;
    }
    if (L == 0) return;
    const int anchor_frame = (int)anchors[tub * 3];      // int(an[t, 0])
    const double dl = (double)L;
    float *xt = x + base * ch.n;
    int run = 0;
    for (int64_t fb = 0; fb < Fv; fb += 64) {
        const int64_t f = fb + lane;
        bool has = false;
        if (f < Fv) {
            const float r0 = tracks[(base + f) * 5];
            has = !(r0 != r0);
        }
        const unsigned long long m = __ballot(has);
        if (has) {
            const int j = run + __popcll(m & ((1ull << lane) - 1ull));
            frames[base + j] = (int32_t)f;
            const double rel = (double)((int)f + 1 - anchor_frame) / dl;
            const double go = gt_overlap ? gt_overlap[base + f] : 0.0;
            for (int q = 0; q < ch.n; ++q) {
                float val;
                switch (ch.code[q]) {
                case kChDet: val = det64 ? (float)det64[base + f] : det32[base + f]; break;
                case kChTrack: val = tracks[(base + f) * 5 + 4]; break;
                case kChAnchor: val = (float)rel; break;
                case kChAbsAnchor: val = (float)fabs(rel); break;
                case kChGtOverlap: val = (float)go; break;
                default: val = go >= 0.5 ? 1.0f : 0.0f; break;
                }
                xt[(int64_t)q * L + j] = val;
            }
        }
        run += __popcll(m);
    }
}

// ------------------------------------------------------------------------------------------------
// The network: one workgroup per tubelet (grid-stride over the tubelets), every layer in this one launch.
// The series is cut into tiles of `tile` positions; a tile's input is staged with a halo of the net's receptive radius and
// the activations of consecutive layers ping-pong between two buffers of maxc x (tile + 2*halo) floats: in LDS
// (GLOBAL = false), or in a per-workgroup slice of a global scratch for nets too wide for the LDS budget (GLOBAL = true,
// same code, same results).  Positions of a halo that lie outside the series are ZERO at every layer ("same" padding).
// Weights are not staged: the output channel is wave-uniform, so w and b come through scalar loads / the constant cache
// once per (wave, output channel), not once per output element.
// x: channel-major [cin, L] at tub_base*cin; frames (may be null: identity) at tub_base; out[tub_base + frame] = probs[1].
// ------------------------------------------------------------------------------------------------
template <bool GLOBAL>
__global__ __launch_bounds__(kTcnThreads) void tcn_net_kernel(TcnNet net, const float *__restrict__ params, const float *__restrict__ x,
                                                              const int32_t *__restrict__ frames, const int64_t *__restrict__ tub_base,
                                                              const int32_t *__restrict__ tub_len, int64_t ntub, int tile,
                                                              float *__restrict__ scratch, float *__restrict__ out)
{
    extern __shared__ float tcn_lds[];
    const int wt = tile + 2 * net.halo;
    const int bufsz = net.maxc * wt;
    float *buf0 = GLOBAL ? scratch + (size_t)blockIdx.x * 2 * bufsz : tcn_lds;
    float *buf1 = buf0 + bufsz;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    constexpr int nwaves = kTcnThreads / 64;
    for (int64_t tub = blockIdx.x; tub < ntub; tub += gridDim.x) {
        const int L = tub_len[tub];
        if (L <= 0) continue;
        const int64_t base = tub_base[tub];
        const float *xt = x + base * net.cin;
        for (int s = 0; s < L; s += tile) {
            const int e = min(s + tile, L);
            const int org = s - net.halo;              // series position of buffer index 0
            const int w0 = (e - s) + 2 * net.halo;     // staged width of this tile
            __syncthreads();                           // the previous tile / tubelet is done with the buffers
            for (int i = tid; i < net.cin * w0; i += kTcnThreads) {
                const int ci = i / w0, p = i - ci * w0 + org;
                buf0[ci * wt + (p - org)] = (p >= 0 && p < L) ? xt[(int64_t)ci * L + p] : 0.0f;
            }
            __syncthreads();
            float *in = buf0, *ob = buf1;
            for (int li = 0; li < net.n; ++li) {
                const TcnLayer ly = net.l[li];
                const int h = ly.k / 2;
                const int lo = s - ly.rem, hi = e + ly.rem;          // output positions of this layer
                const bool last = li == net.n - 1;
                for (int co = wave; co < ly.cout; co += nwaves) {
                    const float *w = params + ly.woff + (size_t)co * ly.cin * ly.k;
                    const float bias = params[ly.boff + co];
                    for (int p = lo + lane; p < hi; p += 64) {
                        float acc = 0.0f;
                        if (p >= 0 && p < L) {
                            acc = bias;
                            const float *ip = in + (p - h - org);
                            for (int ci = 0; ci < ly.cin; ++ci)
                                for (int k = 0; k < ly.k; ++k) {
                                    const float pr = w[ci * ly.k + k] * ip[ci * wt + k];
                                    acc = acc + pr;
                                }
                            if (!last) acc = acc > 0.0f ? acc : 0.0f;
                        }
                        ob[co * wt + (p - org)] = acc;
                    }
                }
                __syncthreads();
                float *sw = in; in = ob; ob = sw;
            }
            // channel softmax of the last layer's output (softmax_channels_kernel), probs[1] to the box's frame; a net of
            // zero layers (the wide first layer was the only one) is this stage alone on its staged input
            const int cl = net.n ? net.l[net.n - 1].cout : net.cin;
            for (int p = s + tid; p < e; p += kTcnThreads) {
                const float *a = in + (p - org);
                float m = a[0];
                for (int cc = 1; cc < cl; ++cc) m = fmaxf(m, a[cc * wt]);
                float sum = 0.0f;
                for (int cc = 0; cc < cl; ++cc) sum = sum + expf(a[cc * wt] - m);
                const float pr = expf(a[wt] - m) / sum;
                const int64_t f = frames ? (int64_t)frames[base + p] : (int64_t)p;
                out[base + f] = pr;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// The wide first layer: layer 0 of a net whose input has per-box ROWS (all_scores [.., 200], feats [.., 1024]) beside, or
// instead of, the assembled one-value-per-box channels.  The input is a table of segments in the net's `inputs` order; a wide
// segment is read where the caller left it, rows [boxes, width] in the tracks' box order, gathered through the frame list:
// a row is read only for a box of the series, so rows of holes and of slots behind ntracks are never touched.
//
// Grid (tubelets (grid-stride), position tiles (grid-stride)); a workgroup computes every output channel of one tile of
// kTcnWideTile = 128 positions, two per lane (lane and lane + 64).  The concatenated channels pass through LDS in chunks of
// kTcnWideChunk = 32:
//   staging  a half wave takes a row (a position of tile + halo), its 32 lanes consecutive channels of it -- consecutive
//            addresses of the caller's tensor, by ELEMENT loads, because row bases are only element-aligned (odd widths,
//            16-bit storage, views); the call is bound by its multiply-adds (cout * K of them per element), not by these
//            loads -- and writes tile[channel][position]; the pitch is ODD, so the 32 lanes, one pitch apart each, fall on
//            32 different banks (bank = dword address % 32 for ds_write_b32, conflicts per 32-lane half);
//   compute  a lane reads tile[ci][lane + k] and [lane + 64 + k]: consecutive dwords over the lanes, conflict-free at any pitch.
// A wave owns A consecutive output channels, so a lane carries 2A accumulators: two LDS reads and A scalar weights feed A
// packed multiplies and A packed adds (the two positions of a lane are the two halves; every product and every sum is
// rounded on its own, nothing is fused or reassociated).  The four waves cover 4A channels; a layer with more takes further
// passes over the tile, whose rows then come from L2 again.  The accumulators stay in registers across all chunks of a pass,
// because every chain is sequential in ci.  W0[co] is contiguous in ci*K + k and comes through scalar loads; with K a template
// parameter (3, 5) two channels' taps of one output channel are one run of 2K dwords, which the compiler loads in wide
// pieces; any other K takes the generic instantiation (KT = 0), one scalar dword per weight.
// Arithmetic = conv1d_kernel's: acc = b[co]; ci ascending over the concatenation, k inner; p = w * x rounded, acc = acc + p; a
// position outside the series is staged as +0.0f and its product IS added.  h0 [cout, L] channel-major at tub_base * cout.
// ------------------------------------------------------------------------------------------------
constexpr int kTcnMaxSegs = 16;          // inputs of one call, one-channel and wide together
constexpr int kTcnWideTile = 128;        // positions of one tile of the wide first layer: two per lane
constexpr int kTcnWideChunk = 32;        // channels staged at a time: one per lane of a staging half wave
constexpr int kTcnWidePitch = (kTcnWideTile + 2 * (kTcnMaxK / 2)) | 1;   // largest (odd) pitch: 159 floats

enum { kTcnRowF32 = 0, kTcnRowF16 = 1, kTcnRowBF16 = 2, kTcnRowF64 = 3, kTcnRowTypes = 4 };   // storage of wide rows

struct TcnSeg {
    const void *rows;    // wide: the caller's rows [boxes, width]; null: channel `xq` of the assembled x
    int32_t width;       // channels of the segment (1 for an assembled channel)
    int32_t dtype;       // kTcnRow*
    int32_t c0;          // first channel of the segment in the concatenation
    int32_t xq;
};

typedef float tcn_f2 __attribute__((ext_vector_type(2)));

// one element of a wide row as f32: f16 / bf16 widen exactly, f64 rounds once to nearest (np.asarray(.., dtype='float32'))
__device__ __forceinline__ float tcn_row_elem(const void *rows, int dtype, int64_t i)
{
    switch (dtype) {
    case kTcnRowF32: return static_cast<const float *>(rows)[i];
    case kTcnRowF16: return (float)static_cast<const _Float16 *>(rows)[i];
    case kTcnRowBF16: return __uint_as_float((uint32_t) static_cast<const uint16_t *>(rows)[i] << 16);
    default: return (float)static_cast<const double *>(rows)[i];
    }
}

// NT consecutive weights of each of the A output channels (t = ci*K + k onward) against the NT staged values xv, in order
template <int A, int NT>
__device__ __forceinline__ void tcn_wide_mac(tcn_f2 (&acc)[A], const float *const (&wr)[A], int t, const tcn_f2 (&xv)[NT])
{
#pragma unroll
    for (int a = 0; a < A; ++a) {
        const float *w = wr[a] + t;
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const tcn_f2 pr = w[i] * xv[i];
            acc[a] = acc[a] + pr;
        }
    }
}

template <int A, int KT>
__global__ __launch_bounds__(kTcnThreads) void tcn_wide_layer_kernel(const TcnSeg *__restrict__ segs, int nseg, int cin, int cout, int krt,
                                                                     int relu, const float *__restrict__ w0, const float *__restrict__ b0,
                                                                     const float *__restrict__ x, int nx, const int32_t *__restrict__ frames,
                                                                     const int64_t *__restrict__ tub_base, const int32_t *__restrict__ tub_len,
                                                                     int64_t ntub, float *__restrict__ h0)
{
    __shared__ float tile[kTcnWideChunk * kTcnWidePitch];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    constexpr int nwaves = kTcnThreads / 64;
    const int K = KT ? KT : krt;
    const int h = K / 2;
    const int w0n = kTcnWideTile + 2 * h;       // staged positions: the tile and its halo
    const int pitch = w0n | 1;
    const int npass = (cout + A * nwaves - 1) / (A * nwaves);
    for (int64_t tub = blockIdx.x; tub < ntub; tub += gridDim.x) {
        const int L = tub_len[tub];
        if (L <= 0) continue;
        const int64_t base = tub_base[tub];
        for (int64_t s64 = (int64_t)blockIdx.y * kTcnWideTile; s64 < L; s64 += (int64_t)gridDim.y * kTcnWideTile) {
            const int s = (int)s64, org = s - h;           // series position of tile column 0
            for (int pass = 0; pass < npass; ++pass) {
                const int co0 = (pass * nwaves + wave) * A;
                const bool live = co0 < cout;              // wave-uniform
                tcn_f2 acc[A];
                const float *wr[A];                        // rows of W0 [cout, cin*K]; channels past cout repeat the last one
#pragma unroll
                for (int a = 0; a < A; ++a) {
                    const int co = min(co0 + a, cout - 1);
                    wr[a] = w0 + (size_t)co * cin * K;
                    acc[a] = b0[co];
                }
                for (int g0 = 0; g0 < cin; g0 += kTcnWideChunk) {
                    const int cw = min(kTcnWideChunk, cin - g0);
                    __syncthreads();                       // the previous chunk / pass / tile is read
                    for (int sg = 0; sg < nseg; ++sg) {
                        const TcnSeg S = segs[sg];
                        const int qa = max(S.c0, g0), qb = min(S.c0 + S.width, g0 + cw);
                        if (qa >= qb) continue;
                        if (!S.rows) {
                            const float *xc = x + base * nx + (int64_t)S.xq * L;
                            float *tc = tile + (qa - g0) * pitch;
                            for (int j = tid; j < w0n; j += kTcnThreads) {
                                const int p = org + j;
                                tc[j] = (p >= 0 && p < L) ? xc[p] : 0.0f;
                            }
                        } else {
                            const int q = qa + (lane & 31);
                            for (int j = 2 * wave + (lane >> 5); j < w0n; j += 2 * nwaves) {
                                const int p = org + j;
                                if (q < qb) {
                                    float v = 0.0f;
                                    if (p >= 0 && p < L)
                                        v = tcn_row_elem(S.rows, S.dtype, (base + (int64_t)frames[base + p]) * S.width + (q - S.c0));
                                    tile[(q - g0) * pitch + j] = v;
                                }
                            }
                        }
                    }
                    __syncthreads();
                    if (live) {
                        const float *tp = tile + lane;
                        int t = g0 * K, ci = 0;
                        if (KT) {
                            constexpr int KK = KT ? KT : 1;
                            for (; ci + 2 <= cw; ci += 2, tp += 2 * pitch, t += 2 * KK) {
                                tcn_f2 xv[2 * KK];
#pragma unroll
                                for (int k = 0; k < KK; ++k) {
                                    xv[k] = tcn_f2{tp[k], tp[k + 64]};
                                    xv[KK + k] = tcn_f2{tp[pitch + k], tp[pitch + k + 64]};
                                }
                                tcn_wide_mac<A, 2 * KK>(acc, wr, t, xv);
                            }
                            for (; ci < cw; ++ci, tp += pitch, t += KK) {
                                tcn_f2 xv[KK];
#pragma unroll
                                for (int k = 0; k < KK; ++k) xv[k] = tcn_f2{tp[k], tp[k + 64]};
                                tcn_wide_mac<A, KK>(acc, wr, t, xv);
                            }
                        } else {
                            for (; ci < cw; ++ci, tp += pitch)
                                for (int k = 0; k < K; ++k, ++t) {
                                    const tcn_f2 xv[1] = {tcn_f2{tp[k], tp[k + 64]}};
                                    tcn_wide_mac<A, 1>(acc, wr, t, xv);
                                }
                        }
                    }
                }
                if (live) {
#pragma unroll
                    for (int a = 0; a < A; ++a) {
                        if (co0 + a >= cout) break;
                        float *ho = h0 + base * cout + (int64_t)(co0 + a) * L;
                        const int p0 = s + lane, p1 = p0 + 64;
                        if (p0 < L) ho[p0] = (relu && !(acc[a].x > 0.0f)) ? 0.0f : acc[a].x;
                        if (p1 < L) ho[p1] = (relu && !(acc[a].y > 0.0f)) ? 0.0f : acc[a].y;
                    }
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Ground-truth overlap: grid (C*T, V), one wave per tubelet slot, lanes over the frames.
//   gt_overlap[b + f] = max over the ground-truth boxes g of (video, frame f + 1, class slot) of iou([g], [box]) in f64
//                       (iou_f64_pair(g, box): the operand order of utils/protocol.py:483), 0.0 when there is none or none
//                       is larger than 0 (a NaN IoU never wins), NaN where the tubelet has no box;
//   mean_iou[tub]     = the f64 mean over the tubelet's boxes, summed sequentially in frame order (NaN: no tubelet);
//   gt[tub]           = |mean - 1| < DBL_EPSILON.
// The box is the f32 track row (or boxes[.., 4] when given) converted to f64 WITHOUT truncation -- the values the device
// evaluator matches; a tracks_to_proto box is int()-truncated, so the two agree on integer-valued boxes only.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void tubelets_overlap_kernel(EvGt g, const int64_t *__restrict__ foff, int64_t F1,
                                                              const int32_t *__restrict__ vid, int vid1, int C, int T,
                                                              const float *__restrict__ tracks, const float *__restrict__ boxes,
                                                              const int32_t *__restrict__ ntracks, const int32_t *__restrict__ col_slot,
                                                              double *__restrict__ gt_overlap, double *__restrict__ mean_iou,
                                                              int32_t *__restrict__ gt_flag)
{
    const int lane = threadIdx.x;
    const int v = blockIdx.y;
    const int ct = blockIdx.x, c = ct / T, t = ct - c * T;
    const int64_t f0 = foff ? foff[v] : 0, Fv = foff ? foff[v + 1] - f0 : F1;
    const int64_t base = (int64_t)C * T * f0 + (int64_t)ct * Fv;
    const int64_t tub = (int64_t)v * C * T + ct;
    const int vi = vid ? vid[v] : vid1;
    const int slot = col_slot[c];
    int nt = ntracks[(int64_t)v * C + c];
    nt = nt < 0 ? 0 : (nt > T ? T : nt);
    const double qnan = __builtin_nan("");
    for (int64_t f = lane; f < Fv; f += 64) {
        const float r0 = tracks[(base + f) * 5];
        double best = qnan;
        if (t < nt && !(r0 != r0)) {
            const float *bp = boxes ? boxes + (base + f) * 4 : tracks + (base + f) * 5;
            const double q[4] = {(double)bp[0], (double)bp[1], (double)bp[2], (double)bp[3]};
            int g0, ng;
            ev_gt_range(g, vi, f + 1, slot, g0, ng);
            best = 0.0;
            for (int j = 0; j < ng; ++j) {
                const double val = iou_f64_pair(g.boxes + (int64_t)(g0 + j) * 4, q);
                if (val > best) best = val;
            }
        }
        gt_overlap[base + f] = best;
    }
    __syncthreads();
    if (lane == 0) {
        double sum = 0.0;
        int L = 0;
        for (int64_t f = 0; f < Fv; ++f) {
            const double o = gt_overlap[base + f];
            const float r0 = tracks[(base + f) * 5];
            if (t < nt && !(r0 != r0)) { sum = sum + o; ++L; }
        }
        const double mean = L ? sum / (double)L : qnan;
        mean_iou[tub] = mean;
        gt_flag[tub] = (L && fabs(mean - 1.0) < 2.220446049250313e-16) ? 1 : 0;
    }
}

}  // namespace vdet
