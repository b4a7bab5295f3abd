// vdet_capi.hip -- C-ABI of libvdet_hip.so (see include/vdet_hip.h) and the host-side
// orchestration of the gfx950 kernels.  Built with
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -shared
// (-ffp-contract=off is load-bearing: the f32 operation order of the IoU predicate is the spec).
#include <hip/hip_runtime.h>
#include <atomic>
#include <chrono>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/vdet_hip.h"
#include "nms_kernels.hpp"
#include "binsort_kernels.hpp"
#include "small_kernels.hpp"
#include "detnms_kernels.hpp"
#include "decode_kernels.hpp"
#include "proposal_kernels.hpp"
#include "fused_kernels.hpp"
#include "adjrows_kernels.hpp"
#include "graphlists_kernels.hpp"
#include "temporal_kernels.hpp"
#include "tubelet_kernels.hpp"
#include "track_kernels.hpp"
#include "batch_kernels.hpp"
#include "gemm_kernels.hpp"
#include "eval_kernels.hpp"
#include "tcn_kernels.hpp"
#include "interp_kernels.hpp"
#include "anchor_kernels.hpp"
#include "topanchor_kernels.hpp"
#include "context_kernels.hpp"
#include "merge_kernels.hpp"
#include "tubenms_kernels.hpp"
#include "tracknms_kernels.hpp"
#include "softnms_kernels.hpp"
#include "votenms_kernels.hpp"
#include "rescore_kernels.hpp"
#include "patch_kernels.hpp"
#include "roipool_kernels.hpp"
#include "svmhead_kernels.hpp"
#include "pixtrack_kernels.hpp"
#include "motion_kernels.hpp"
#include "seqnms_kernels.hpp"

using namespace vdet;

namespace {

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    hipError_t reserve(size_t bytes)
    {
        if (bytes <= cap) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        size_t want = bytes + bytes / 4 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) {  // retry exact
            want = bytes;
            e = hipMalloc(&p, want);
        }
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    template <typename T> T *as() { return static_cast<T *>(p); }
};

enum Stage { ST_IOU_BITS = 0, ST_ADJ = 1, ST_SORTK = 2, ST_WALK = 3, ST_TEMPORAL = 4, ST_SORT = 5, ST_IOU_GEN = 6, ST_OTHER = 7,
             ST_TRANSPOSE = 8, ST_TPICK = 9, ST_TLINK = 10, ST_TSUPP = 11, ST_RSPATIAL = 12, ST_RSERIES = 13, ST_SORTFB = 14, ST_TLOOP = 15, ST_COUNT = 16 };

struct Counters {            // one small device block
    // sticky until vdet_sync (or a synchronous graph build) reads and clears them
    int status;
    int eindex;              // latched "IndexError" of the rescoring kernels
    unsigned long long pool_max;   // largest pool_used of the asynchronous builds since the last vdet_sync
    // per graph build (kPerBuildOff .. end): cleared when a build starts
    unsigned int glob_cnt;
    int irregular;           // frames that are not "regular" (frame_flags_kernel), counted per graph build
    unsigned long long pool_used;
};
constexpr size_t kPerBuildOff = 16;

// an asynchronous build is about to clear the per-build counters: keep the largest pool demand of the window
__global__ void fold_pool_kernel(Counters *cnt)
{
    if (cnt->pool_used > cnt->pool_max) cnt->pool_max = cnt->pool_used;
}

// a small host table the device reads in an asynchronous call: the host copy lives in the context so it outlives the copy made
// from it, and a call that brings the same bytes again uploads nothing (stage_table / stage_keyed)
struct StagedTab {
    DevBuf dev;
    std::vector<char> host;       // what the device holds (the source of the last copy)
    std::vector<char> key;        // stage_keyed: the bytes the table was built from, compared instead of the table itself
    bool valid = false;
    long long uploads = 0;        // copies made so far
};

// which sorted lists c->order / c->ncand hold (thr takes part only under use_thr)
struct ListsKey {
    const void *scores = nullptr;
    int64_t C = 0;
    int layout = -1, use_thr = 0;
    float thr = 0;
    int topk = 0;
    bool operator==(const ListsKey &o) const { return scores == o.scores && C == o.C && layout == o.layout && use_thr == o.use_thr && (!use_thr || thr == o.thr) && topk == o.topk; }
};

struct NmsPlan {
    std::vector<GroupDesc> groups;   // bits_off is batch-local
    std::vector<TileDesc> tiles;     // ordered by batch
    std::vector<TilePair> pairs;     // upper-triangle 256x256 tile pairs, ordered by batch
    std::vector<std::pair<int, int>> batch_tiles;  // [t0, t1) per batch
    std::vector<std::pair<int, int>> batch_pairs;  // [p0, p1) per batch
    std::vector<ListItem> ditems;    // direct lists (graph_lists_kernel): one work item per (row tile, width quartile)
    std::vector<std::pair<int, int>> batch_ditems;
    size_t bits_words_max = 0;       // largest batch
    int64_t ntot = 0;
    int nmax = 0;
};


}  // namespace

struct vdet_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t own_stream = nullptr;
    std::string err;
    Counters *d_cnt = nullptr;
    int latched = 0;              // first failure latched by async entry points
    size_t bits_budget = (size_t)1 << 30;
    size_t max_lds = 160 * 1024;
    int n_cu = 256;
    // scratch
    DevBuf boxes, scores, keys, excl, frames, groups, tiles, bits, rowz, rowmeta, groupz, adj, comp, origidx,
        out64, trk_frames, trk_boxes, b1, b2, iou_out, order, ncand, keepidx, keepcnt, gflags, pairs, tkeys, tstate, visited, heads, xkeys, xord, wmeta, wmeta16, reachtab, rowperm, qreach, ditems, striptot, stripoff, xncand, xbox, xbox16, xord16, xcum, xinfo, tmp[8];
    // timing
    bool timing = false;
    bool timing_accumulate = false;   // vdet_set_timing(ctx, 2): keep events across calls until read
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
    std::vector<int> ev_stage;
    size_t ev_used = 0;
    float last_ms[ST_COUNT] = {0};
    int last_launches[ST_COUNT] = {0};
    bool sort_attr_set = false;
    // opt-in reuse of the per-video preparation (graph + sorted lists) between d_* calls
    // (owned by the prep-cache helpers next to volume_plan: nothing else reads prep or sets a flag; anyone may clear one)
    bool cache_enabled = false;
    struct PrepKey { const void *boxes = nullptr; int64_t F = 0, B = 0; float t32 = 0; ListsKey lists; } prep;
    bool graph_valid = false, lists_valid = false;
    // class-major sort keys left in c->tkeys by vdet_volume_pass (reused like the other prep, cache on)
    struct KeySrc { const void *scores = nullptr; int64_t F = 0, B = 0, C = 0; int use_thr = 0; float thr = 0; } keysrc;
    bool keys_valid = false;
    bool vpass_attr_set = false;
    int vpass_form = VDET_VPASS_AUTO;   // vdet_set_vpass / VDET_VPASS_FORM: which form of the volume pass (include/vdet_hip.h)
    int vpass_fchunk = 0;               // ... and frames per chunk (0: the host's formula); VDET_VPASS_FCHUNK
    int vpass_last_items = 0;           // vdet_query 12: items per thread of the last volume pass's fused kernel (0: the separate kernels
                                        // ran), + 100 if it was held to one block per compute unit
    bool index_valid = false; const void *index_boxes = nullptr; int64_t index_F = 0, index_B = 0;
    bool all_regular = false;     // last graph build: every frame regular
    bool wave_transpose = false;  // wave_transpose64 verified on this device (vdet_create); VDET_WAVE_TRANSPOSE=0 disables
    // Diagnostic switches (read once at vdet_create; DESIGN.md "Knobs").  Each forces a FALLBACK path the library takes anyway
    // on some inputs or devices, so that the tests can run it on every input: no tuning variants live here.
    bool no_lazy = false;         // VDET_NO_LAZY=1: eager track_det_nms of every crossed list (the irregular-frame path)
    bool no_index = false;        // VDET_NO_INDEX=1: no x-sorted proposal index (the path of frames too large for it)
    bool force_general = false;   // VDET_FORCE_GENERAL=1: the general predicate kernel K1 on every frame (the irregular-frame path)
    bool atomic_rank = false;     // LDS returning atomics serve same-address lanes in lane order (probed; VDET_ATOMIC_RANK=0: ballot match)
    bool small_lists = true;      // VDET_SMALL_LISTS=0: frames of <= 384 boxes through the large-list sort and walk too (small_kernels.hpp)
    bool adj_rows = true;         // VDET_ADJ_ROWS=0: adj_build_kernel (a lane per row) also for the regular frames of large volumes
    bool direct_lists = true;     // VDET_DIRECT_LISTS=0: regular frames through the bit matrix + adj_rows_kernel (also taken, for good,
                                  // once a row had more neighbours than a direct slot holds)
    uint32_t direct_cap = 384;    // entries per row slot of the direct lists (a multiple of 8)
    int64_t direct_ntot = 0;      // rows / fixed part of the pool of the last direct build (the failure path sizes the pool from them)
    unsigned long long direct_fixed = 0;
    bool no_fused = false;        // VDET_NO_FUSED=1: the host-buffer calls of <= 640 rows through the general kernel chain too (the path of larger inputs)
    bool binsort = true;          // VDET_BINSORT=0: the LSD radix kernel (the fallback of tied / thresholded columns) for every column
    bool binsort_inherit = true;  // VDET_BINSORT_INHERIT=0: every column of the counting sort builds its own key -> bin map
    int binsort_grid = 0;         // VDET_BINSORT_GRID=n: at most n workgroups for the counting sort (0: as many as fit the chip)
    const std::vector<GroupDesc> *host_groups = nullptr;   // group table of the call in flight (mode 2)
    bool sym_built = false;       // the last graph build ran K0 + frame index + K1s (regular-frame fast path)
    // volume geometry whose group / tile / pair tables are resident in c->groups / c->tiles / c->pairs
    // (uploaded once per geometry: the host copy lives here so no call has to wait for the copies)
    NmsPlan vplan;
    bool vplan_valid = false;     // ... and the device tables still hold it
    int64_t vplan_F = 0, vplan_B = 0;
    size_t vplan_budget = 0;
    // asynchronous video step (vdet_set_async): no host synchronisation inside the d_* entry points
    long long n_host_syncs = 0;   // hipStreamSynchronize calls made by this context so far
    bool async_enabled = false;
    unsigned long long pool_hint = 0;   // adjacency entries used by the largest graph built so far
    bool topk_attr_set = false;
    float gt32 = 0.f;             // threshold of the last graph build (the packed walk's in-group test)
    bool wmeta16_built = false;   // ... and adj_rows_kernel the 16-byte form of the records of integer frames
    bool wmeta_built = false;     // ... which also wrote the packed walk's records (WalkMeta) of the regular frames
    bool last_sort_binned = false;   // the last per-(frame, class) sort went through binsort_kernel (vdet_query 9)
    StagedTab vidtab, segtab;     // batched videos, keyed by the frame offsets: {first frame, frames} per video / per frame {first, one past last} of its video
    DevBuf sortctl;               // binsort_kernel's work counter + the list of problems it handed to the LSD kernel
    int walk_wide_nsw = 12;       // the packed walk filters its lists' sparse tails kWideW chunks per pass once a pass queued fewer
                                  // candidates than this (VDET_WALK_WIDE=0: never; VDET_WALK_WIDE_NSW: 1..63)
    bool last_walk_wide = false;  // the last walk could take the wide filter (vdet_query 18 / 19)
    DevBuf walkstats;             // [2][kWideStatSlots] u32: lists that went wide / wide passes that overflowed in the last walk
    DevBuf nover;                 // vdet_det_nms_volume: candidates per list before the topk cut
    DevBuf ordncand;              // vdet_nms_volume_ordered: the caller's counts after check_order_kernel
    DevBuf linkmemo, linkstats, linkwarm, linkorder, linkchains, linknodes, tracknode, rtodo;
    // which proposal every row of the last tracking call's tracks is (written by the link kernels; vdet_rescore_tracks
    // then finds a tubelet box's overlapping detections among that proposal's graph neighbours)
    struct NodeKey { const void *tracks = nullptr, *boxes = nullptr; int64_t F = 0, B = 0, C = 0; int T = 0; double nms_thres = 0; } nodekey;
    bool nodes_valid = false;
    // single-launch drop-in calls (vdet_nms_f32 / vdet_track_det_nms_f32 on <= kFusedMax rows): host-mapped staging
    void *fused_in = nullptr, *fused_out = nullptr;          // host addresses
    void *fused_in_dev = nullptr, *fused_out_dev = nullptr;  // ... and what the device calls them
    void *fbatch_in = nullptr, *fbatch_out = nullptr, *fbatch_in_dev = nullptr, *fbatch_out_dev = nullptr;   // vdet_track_det_nms_batch (grown on demand)
    size_t fbatch_in_cap = 0, fbatch_out_cap = 0;
    bool fbatch_attr = false;
    size_t dyn_lds_max = 0;
    // device evaluator (eval_kernels.hpp): dense per-call match results, compaction counts, radix-sort ping-pong buffers
    DevBuf ev_tab, ev_dtp, ev_dsc, ev_dslot, ev_bcnt, ev_boff, ev_key[2], ev_val[2], ev_hist;
    // device TCN (tcn_kernels.hpp): assembled channels, frame lists, tubelet descriptors, the global-path activations, and the
    // host tables its asynchronous calls read on the device (net parameters, frame offsets, the overlap call's tables)
    DevBuf tcn_x, tcn_frames, tcn_base, tcn_len, tcn_scratch, tcn_h0;      // (tcn_h0: the wide first layer's output)
    StagedTab tcn_params, tcn_foff, tcn_ovtab, tcn_segs;      // (tcn_params.uploads: vdet_query 10)
    bool tcn_tiled = false;       // VDET_TCN_TILED=1: every series cut into the smallest tiles (the path of long series / wide nets)
    bool tcn_global = false;      // VDET_TCN_GLOBAL=1: activations in global memory (the path of nets too wide for the LDS budget)
    StagedTab interp_tab;         // device interpolation (interp_kernels.hpp): frame offsets and the frame table of the last call
    // the per-video {first frame, frames} table of every tubelet-stage batch form (anchor selection and route, merge, tubelet
    // NMS, re-scoring, Seq-NMS), keyed by the frame offsets (video_table; anchor_tab.uploads: vdet_query 11), and the scratch of
    // the device anchor selection (topanchor_kernels.hpp)
    StagedTab anchor_tab;
    DevBuf topa_hist, topa_state, topa_cnt, topa_nrec, topa_rec;
    bool topa_hist_clean = false; // the histogram holds zeros (every selection round clears what it read)
    DevBuf svm_wt, svm_wavebad;   // SVM head (svmhead_kernels.hpp): the W^T copy of the call and the per-wave counts of empty groups
    // multi-context suppression (context_kernels.hpp): the per-video {elements, record slice} table of the batch forms, keyed by
    // the offsets and the shape, and the selection's scratch
    StagedTab ctxs_tab;
    DevBuf ctxs_hist, ctxs_state, ctxs_rec;
    int64_t ctxs_last_videos = 0; // videos of the last vdet_context_classes (vdet_query 13)
    bool ctxs_records = true;     // VDET_CTX_RECORDS=0: no record scratch, every video through the full-read passes (the path of a video
                                  // whose records outgrow it twice: an all-equal volume)
    // Seq-NMS (seqnms_kernels.hpp): the link bits, the live bits, the done flags and -- for videos whose predecessor table
    // outgrows the LDS -- the table itself
    DevBuf sq_link, sq_live, sq_done, sq_ptr;
    bool sq_lds = true;           // VDET_SEQNMS_LDS=0: the predecessor table in global scratch (the path of long videos)
    bool sq_attr_set = false;
    int sq_last_path = -1;        // vdet_query 14: 1 the table in LDS, 2 in global scratch
    // RPN proposal layer (proposal_kernels.hpp): keys and boxes of every anchor, then per frame the candidates in order (boxes,
    // scores, indices, the identity order list, the count) and the NMS keep list over them
    DevBuf rpn_keys, rpn_boxes, rpn_cbox, rpn_cscore, rpn_cindex, rpn_order, rpn_ccnt, rpn_keep, rpn_keepcnt;
    bool rpn_attr_set = false;
    DevBuf tube_scratch;          // NMS over whole tubelets (tubenms_kernels.hpp): scores, counts, extents and the bit rows per (video, class)
};

namespace {

// every host wait of the library goes through here (counted: vdet_query(ctx, 8); the asynchronous video step is
// tested to add none)
hipError_t host_sync(vdet_ctx *c)
{
    ++c->n_host_syncs;
    return hipStreamSynchronize(c->stream);
}

int fail(vdet_ctx *c, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    return code;
}

#define HIPCHK(c, expr)                                                                          \
    do {                                                                                         \
        hipError_t _e = (expr);                                                                  \
        if (_e != hipSuccess)                                                                    \
            return fail((c), VDET_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

struct StageTimer {
    vdet_ctx *c;
    size_t slot = (size_t)-1;
    StageTimer(vdet_ctx *ctx, int stage) : c(ctx)
    {
        if (!c->timing) return;
        if (c->ev_used == c->ev_pool.size()) {
            hipEvent_t a, b;
            if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
            c->ev_pool.push_back({a, b});
            c->ev_stage.push_back(0);
        }
        slot = c->ev_used++;
        c->ev_stage[slot] = stage;
        (void)hipEventRecord(c->ev_pool[slot].first, c->stream);
    }
    ~StageTimer()
    {
        if (slot != (size_t)-1) (void)hipEventRecord(c->ev_pool[slot].second, c->stream);
    }
};

void timing_reset(vdet_ctx *c) { if (!c->timing_accumulate) c->ev_used = 0; }

// StagedTab, the miss: fill(host bytes) writes the new table.  A change waits for the stream once (the copy made from the old
// bytes may be in flight); the table is resident only once its copy is enqueued, so a failed reserve or copy leaves none.
template <typename Fill> int stage_upload(vdet_ctx *c, StagedTab &t, size_t bytes, Fill fill)
{
    t.valid = false;
    if (!t.host.empty()) HIPCHK(c, host_sync(c));
    t.host.resize(bytes);
    fill(t.host.data());
    HIPCHK(c, t.dev.reserve(std::max<size_t>(bytes, 16)));
    if (bytes) HIPCHK(c, hipMemcpyAsync(t.dev.p, t.host.data(), bytes, hipMemcpyHostToDevice, c->stream));
    t.valid = true;
    ++t.uploads;
    return VDET_OK;
}

// the table IS the caller's bytes: the same bytes again cost neither a wait nor a copy
int stage_table(vdet_ctx *c, StagedTab &t, const void *src, size_t bytes)
{
    if (t.valid && t.host.size() == bytes && memcmp(t.host.data(), src, bytes) == 0) return VDET_OK;
    return stage_upload(c, t, bytes, [&](char *dst) { memcpy(dst, src, bytes); });
}

// the table is BUILT from the caller's bytes (O(frames) from O(videos) offsets): the same key again does not even build it
template <typename Fill> int stage_keyed(vdet_ctx *c, StagedTab &t, const void *key, size_t key_bytes, size_t bytes, Fill fill)
{
    if (t.valid && t.key.size() == key_bytes && memcmp(t.key.data(), key, key_bytes) == 0) return VDET_OK;
    t.valid = false;
    t.key.assign(static_cast<const char *>(key), static_cast<const char *>(key) + key_bytes);
    return stage_upload(c, t, bytes, fill);
}

// THE check of the frame offsets of V concatenated videos: from 0, increasing -- strictly unless allow_empty; max_videos > 0 caps V
int check_frame_off(vdet_ctx *c, const int64_t *h_frame_off, int64_t V, bool allow_empty, int64_t max_videos, int64_t *Ftot, int64_t *Fmax)
{
    if (!h_frame_off || V < 1) return fail(c, VDET_EINVAL, "at least one video with its frame offsets");
    if (max_videos > 0 && V > max_videos) return fail(c, VDET_EINVAL, "at most %lld videos in one call", (long long)max_videos);
    if (h_frame_off[0] != 0) return fail(c, VDET_EINVAL, "frame_off must start at 0");
    *Fmax = 0;
    for (int64_t v = 0; v < V; ++v) {
        const int64_t f = h_frame_off[v + 1] - h_frame_off[v];
        if (f < (allow_empty ? 0 : 1)) return fail(c, VDET_EINVAL, "frame_off must %s", allow_empty ? "not decrease" : "be strictly increasing");
        *Fmax = std::max(*Fmax, f);
    }
    *Ftot = h_frame_off[V];
    return VDET_OK;
}

// the videos of a call, concatenated along the frame axis
struct Videos { const int64_t *off; int64_t V, F, Fmax; };            // F: all frames, Fmax: the longest video's

// THE readers of a call's frame offsets: nothing else calls check_frame_off
int read_videos(vdet_ctx *c, const int64_t *h_frame_off, int64_t V, int64_t max_videos, Videos *vs, bool allow_empty = false)
{
    *vs = Videos{h_frame_off, V, 0, 0};
    return check_frame_off(c, h_frame_off, V, allow_empty, max_videos, &vs->F, &vs->Fmax);
}

// ... where the offsets are optional: without them one video of F frames, with them they must end at F
int read_videos_or_one(vdet_ctx *c, const int64_t *h_frame_off, int64_t V, int64_t F, int64_t max_videos, Videos *vs)
{
    if (!h_frame_off) { *vs = Videos{nullptr, 1, F, F}; return VDET_OK; }
    const int rc = read_videos(c, h_frame_off, V, max_videos, vs);
    if (rc == VDET_OK && vs->F != F) return fail(c, VDET_EINVAL, "frame_off must end at F");
    return rc;
}

// the per-video {first frame, frames} table in t, keyed by the offsets: built and uploaded only when they differ from those of
// the resident one
int stage_video_table(vdet_ctx *c, StagedTab &t, const Videos &vs)
{
    return stage_keyed(c, t, vs.off, (size_t)(vs.V + 1) * 8, (size_t)vs.V * sizeof(VidDesc), [&](char *dst) {
        VidDesc *tab = reinterpret_cast<VidDesc *>(dst);
        for (int64_t v = 0; v < vs.V; ++v) tab[v] = VidDesc{(int32_t)vs.off[v], (int32_t)(vs.off[v + 1] - vs.off[v])};
    });
}

// ... for the kernels that take one video in their arguments: *vids is null for it and nothing is staged
int video_table(vdet_ctx *c, StagedTab &t, const Videos &vs, const VidDesc **vids)
{
    *vids = nullptr;
    if (vs.V == 1) return VDET_OK;
    const int rc = stage_video_table(c, t, vs);
    if (rc == VDET_OK) *vids = t.dev.as<VidDesc>();
    return rc;
}

// THE limit check of a product of caller-supplied sizes: every factor >= 0 and the product <= limit (fits_upto) or < limit
// (fits_below).  The limit is divided, the factors are never multiplied: a product that would wrap int64_t is refused like
// any other that is too large.
bool fits_upto(int64_t limit, std::initializer_list<int64_t> factors)
{
    if (limit < 0) return false;
    bool zero = false;
    for (const int64_t f : factors) {
        if (f < 0) return false;
        if (f == 0) zero = true;
        else limit /= f;          // floor(floor(limit / a) / b) == floor(limit / (a * b))
    }
    return zero || limit >= 1;
}

bool fits_below(int64_t limit, std::initializer_list<int64_t> factors) { return fits_upto(limit - 1, factors); }

// smallest float32 f with (double)f >= thresh: "(double)ovr_f32 >= thresh" <=> "ovr_f32 >= f"
float thresh_to_f32(double thresh)
{
    if (thresh != thresh) return NAN;
    float f = (float)thresh;  // round to nearest
    if ((double)f < thresh) f = nextafterf(f, INFINITY);
    return f;
}

// half the gap between t32 and the float32 below it: where RN(inter / uni) turns from < t32 to >= t32 (pred_sign)
float half_gap(float t32) { return (t32 - nextafterf(t32, 0.0f)) * 0.5f; }

// thresholds the divide-free test of the regular-frame kernels is exact for: hg must be a normal float (so t32 is no
// subnormal) and at most 1 (t32 <= 2^24), so that hg * uni is finite for the unions of a regular frame, which
// frame_flags_kernel keeps finite by bounding the coordinates (an infinite uni would make the margin inf - inf)
bool sym_threshold_ok(float t32) { return t32 > 1e-30f && t32 <= 16777216.0f && std::isnormal(half_gap(t32)); }

uint32_t pow2ceil(uint32_t x)
{
    uint32_t p = 1;
    while (p < x) p <<= 1;
    return p;
}

int translate_status(vdet_ctx *c, int st)
{
    if (st & kStPoolAsync) return fail(c, VDET_EAGAIN, "adjacency pool overflow in an asynchronous graph build: run the calls again");
    if (st & kStBadOrder) return fail(c, VDET_EINVAL, "a caller-supplied candidate list holds a count or a box index out of range");
    if (st & kStBadAnchor) return fail(c, VDET_EINVAL, "an anchor frame lies outside the video");
    if (st & kStBadPixAnchor) return fail(c, VDET_EINVAL, "track_pixels: an anchor frame outside the video, or an anchor box that is not finite, beyond 2^20, empty or wholly outside the image (the slot is written as an empty one)");
    if (st & kStBadMerge) return fail(c, VDET_EINVAL, "merge 'max': two paired tubelets differ in the frames of their boxes or in their anchor frame");
    if (st & kStBadPropagate) return fail(c, VDET_EINVAL, "propagate_boxes: a keep_cnt outside 0..cap, a keep_idx outside 0..B-1, or a source box that is not finite or beyond 2^20 (the source writes NaN rows)");
    if (st & kStBadKeep) return fail(c, VDET_EINVAL, "nms_tracks: a keep_cnt outside 0..cap or a keep_idx outside 0..B-1 (the entry is skipped)");
    if (st & kStPatchCap) return fail(c, VDET_ECAP, "tubelet_patches / tubelet_rois: more present tubelet boxes in the frame range than cap (the first cap windows are valid)");
    if (st & kStSvmBad) return fail(c, VDET_EINVAL, "svm_head: a slot row outside shape or a class column outside W (the group is skipped, nothing is written for it)");
    if (st & kStDecodeBad) return fail(c, VDET_EINVAL, "tubelet_dets: a slot row outside shape or a class column outside K (the row is skipped, nothing is written for it)");
    if (st & kStEvalList) return fail(c, VDET_EINVAL, "a keep list holds a NaN score, an increasing score or a count / box index out of range");
    if (st & kStDivZero) return fail(c, VDET_EDIVZERO, "float division (zero union)");
    if (st & kStCap) return fail(c, VDET_ECAP, "more survivors than the output capacity");
    if (st & kStPool) return fail(c, VDET_EHIP, "internal: adjacency pool overflow");
    return VDET_OK;
}

// ---------------------------------------------------------------------------------------------
// NMS orchestration
// ---------------------------------------------------------------------------------------------
int make_plan(vdet_ctx *c, NmsPlan &pl)
{
    const size_t budget_words = std::max<size_t>(c->bits_budget / 8, 1);
    size_t cur = 0;
    int t0 = 0, p0 = 0, d0 = 0;
    pl.nmax = 0;
    pl.ntot = 0;
    for (size_t g = 0; g < pl.groups.size(); ++g) {
        GroupDesc &gd = pl.groups[g];
        pl.ntot = std::max<int64_t>(pl.ntot, (int64_t)gd.box_off + gd.nbox);
        pl.nmax = std::max(pl.nmax, gd.nbox);
        if (gd.nbox < 2) { gd.bits_off = 0; continue; }       // singletons: no graph
        const size_t words = (size_t)bit_words_of_group(gd.nbox);
        if (cur && cur + words > budget_words) {
            pl.batch_tiles.push_back({t0, (int)pl.tiles.size()});
            pl.batch_pairs.push_back({p0, (int)pl.pairs.size()});
            pl.batch_ditems.push_back({d0, (int)pl.ditems.size()});
            t0 = (int)pl.tiles.size();
            p0 = (int)pl.pairs.size();
            d0 = (int)pl.ditems.size();
            pl.bits_words_max = std::max(pl.bits_words_max, cur);
            cur = 0;
        }
        gd.bits_off = (int64_t)cur;
        cur += words;
        const int nrt = (gd.nbox + kRowsPerTile - 1) / kRowsPerTile;
        for (int rt = 0; rt < nrt; ++rt) pl.tiles.push_back({(int32_t)g, rt});
        for (int rt = 0; rt < nrt; ++rt)
            for (int ct = rt; ct < nrt; ++ct) pl.pairs.push_back({(int32_t)g, (int16_t)rt, (int16_t)ct});
        // (the widest quartile of every tile first: its items run longest)
        for (int q = 3; q >= 0; --q)
            for (int rt = 0; rt < nrt; ++rt) pl.ditems.push_back({(int32_t)g, (int32_t)(4 * rt + q)});
    }
    if ((int)pl.tiles.size() > t0) {
        pl.batch_tiles.push_back({t0, (int)pl.tiles.size()});
        pl.batch_pairs.push_back({p0, (int)pl.pairs.size()});
        pl.batch_ditems.push_back({d0, (int)pl.ditems.size()});
    }
    pl.bits_words_max = std::max(pl.bits_words_max, cur);
    (void)c;
    return VDET_OK;
}

int sort_groups_by_keys(vdet_ctx *c, int G, int nmax, int64_t ntot);

// x1-sorted proposal index of every group (frame), see nms_kernels.hpp.  Needs c->groups uploaded.
// Used by the fast K1 (rank space + tile skipping) and by the LINK kernels (IoU windows).
int build_frame_index(vdet_ctx *c, const float4 *d_boxes, int64_t ntot, int64_t G, int nmax)
{
    if (c->cache_enabled && c->index_valid && c->index_boxes == d_boxes && c->index_F == G && c->index_B == ntot) return VDET_OK;
    c->index_valid = false;
    HIPCHK(c, c->xkeys.reserve((size_t)ntot * 4));
    HIPCHK(c, c->xord.reserve((size_t)ntot * 2));
    HIPCHK(c, c->xncand.reserve((size_t)G * 4));
    HIPCHK(c, c->xbox.reserve((size_t)ntot * 16));
    // compact copy for frames of integer pixel coordinates (kFlagU16): every group at an even position
    HIPCHK(c, c->xbox16.reserve((size_t)(ntot + G + 4) * 8));
    HIPCHK(c, c->xord16.reserve((size_t)(ntot + G + 4) * 2));
    HIPCHK(c, c->xcum.reserve((size_t)G * 257 * 4));
    HIPCHK(c, c->xinfo.reserve((size_t)G * 16));
    StageTimer tm(c, ST_OTHER);
    hipLaunchKernelGGL(xkey_kernel, dim3((unsigned)((ntot + 255) / 256)), dim3(256), 0, c->stream, d_boxes,
                       c->xkeys.as<uint32_t>(), ntot);
    int rc = sort_groups_by_keys(c, (int)G, nmax, ntot);
    if (rc) return rc;
    hipLaunchKernelGGL(frame_index_kernel, dim3((unsigned)G), dim3(256), 0, c->stream, d_boxes, c->groups.as<GroupDesc>(),
                       c->xord.as<uint16_t>(), c->xbox.as<float4>(), c->xcum.as<uint32_t>(), c->xinfo.as<float>(),
                       c->gflags.as<uint32_t>(), c->xbox16.as<uint2>(), c->xord16.as<uint16_t>());
    HIPCHK(c, hipGetLastError());
    c->index_valid = true; c->index_boxes = d_boxes; c->index_F = G; c->index_B = ntot;
    return VDET_OK;
}

FrameIndex frame_index_of(vdet_ctx *c)
{
    return FrameIndex{c->xbox.as<float4>(), c->xord.as<uint16_t>(), c->xcum.as<uint32_t>(), c->xinfo.as<float>(),
                      c->xbox16.as<uint2>(), c->xord16.as<uint16_t>(), 0};
}

// The plan of a regular volume (one group of B boxes per frame).  Built on the host once per geometry
// and kept in the context: the host tables then outlive every asynchronous copy made from them, and a
// video with the geometry of the previous one finds the device tables already in place.
NmsPlan &volume_plan(vdet_ctx *c, int64_t F, int64_t B)
{
    if (c->vplan_F == F && c->vplan_B == B && c->vplan_budget == c->bits_budget && !c->vplan.groups.empty()) return c->vplan;
    (void)host_sync(c);     // (rare: geometry change) copies from the old tables may be in flight
    // the resident group / tile / pair tables are about to describe another geometry: whatever the cache holds (graph, sorted
    // lists, x-index, recorded track nodes) was built -- and is decoded -- with the old tables
    c->graph_valid = c->lists_valid = c->index_valid = c->nodes_valid = false;
    c->vplan = NmsPlan();
    c->vplan.groups.resize((size_t)F);
    for (int64_t f = 0; f < F; ++f) c->vplan.groups[(size_t)f] = {(int32_t)(f * B), (int32_t)B, 0};
    make_plan(c, c->vplan);
    c->vplan_F = F; c->vplan_B = B; c->vplan_budget = c->bits_budget;
    c->vplan_valid = false;
    return c->vplan;
}

// calls that need only the group table of a volume (one group of B boxes per frame) on the device; tiles / pairs follow
// with the next graph build
int volume_groups(vdet_ctx *c, int64_t F, int64_t B)
{
    NmsPlan &pl = volume_plan(c, F, B);
    c->host_groups = &pl.groups;
    HIPCHK(c, c->groups.reserve((size_t)F * sizeof(GroupDesc)));
    if (!c->vplan_valid)
        HIPCHK(c, hipMemcpyAsync(c->groups.p, pl.groups.data(), (size_t)F * sizeof(GroupDesc), hipMemcpyHostToDevice, c->stream));
    return VDET_OK;
}

int build_graph(vdet_ctx *c, const float4 *d_boxes, NmsPlan &pl, float t32, double thresh, bool volume);

// ---- the prep cache: c->prep, graph_valid and lists_valid are read, and set, only here
// Make the resident suppression graph the one of these boxes at this threshold.  reuse: the resident one may serve, when the
// cache is on and its key matches -- the threshold bit for bit, so that a NaN threshold equals itself; *reused says so.
int ensure_volume_graph(vdet_ctx *c, const float *d_boxes, int64_t F, int64_t B, double nms_thres, bool reuse, bool *reused = nullptr)
{
    const float t32 = thresh_to_f32(nms_thres);
    const bool same = reuse && c->cache_enabled && c->graph_valid && c->prep.boxes == d_boxes && c->prep.F == F && c->prep.B == B &&
                      memcmp(&c->prep.t32, &t32, 4) == 0;
    if (reused) *reused = same;
    if (same) return VDET_OK;
    c->graph_valid = c->lists_valid = c->nodes_valid = false;     // (the recorded track nodes point into the lists rewritten now)
    const int rc = build_graph(c, reinterpret_cast<const float4 *>(d_boxes), volume_plan(c, F, B), t32, nms_thres, true);
    if (rc) return rc;
    c->prep.boxes = d_boxes; c->prep.F = F; c->prep.B = B; c->prep.t32 = t32;
    c->graph_valid = true;
    return VDET_OK;
}

// are the resident sorted lists those of key, made on a volume of F x B?
bool lists_match(const vdet_ctx *c, const ListsKey &key, int64_t F, int64_t B) { return c->lists_valid && c->prep.F == F && c->prep.B == B && c->prep.lists == key; }
void set_lists(vdet_ctx *c, const ListsKey &key) { c->prep.lists = key; c->lists_valid = true; }

// vdet_rescore_tracks: do gflags / the x-index describe these boxes (left by the graph build of the same volume)?
bool index_matches(const vdet_ctx *c, const float *d_boxes, int64_t F, int64_t B)
{
    return c->cache_enabled && c->graph_valid && c->index_valid && c->prep.boxes == d_boxes && c->prep.F == F && c->prep.B == B && c->index_boxes == d_boxes;
}

// ... and are these the tracks of the last tracking call on this context, same boxes, with the graph they were made on (same
// threshold) still in place?  Then c->tracknode says which proposal every tubelet box is.
bool nodes_match(const vdet_ctx *c, const float *d_tracks, const float *d_boxes, int64_t F, int64_t B, int64_t C, int T)
{
    const float nt = thresh_to_f32(c->nodekey.nms_thres);
    return c->cache_enabled && c->nodes_valid && c->graph_valid && c->nodekey.tracks == d_tracks && c->nodekey.boxes == d_boxes &&
           c->prep.boxes == d_boxes && c->nodekey.F == F && c->nodekey.B == B && c->nodekey.C == C && c->nodekey.T == T &&
           c->prep.F == F && c->prep.B == B && memcmp(&c->prep.t32, &nt, 4) == 0;
}

// re-scoring may take a tubelet box's candidates from its proposal's graph neighbours: with the regular-frame flags and
// overlap_thres well above the graph's threshold
bool rescore_from_graph(const uint32_t *group_flags, double nms_thres, double overlap_thres)
{
    return group_flags && overlap_thres - nms_thres > 0.05 && nms_thres > 0.0 && overlap_thres < 1.0;
}

// ---- the tracking workspace of the greedy volume trackers: vdet_nms_track_volume and vdet_track_volume_pixels (n_states = C),
// vdet_video_batch (n_states = V * C)
struct TrackWork {
    const uint32_t *flags;        // regular-frame flags, or null: only when the graph in place ran K0 + the frame index
    FrameIndex ix;                // ... and the x-index for the link windows, when there is one
    bool filled;                  // small frames: the whole link table is filled up front, nothing is predicted
    float link_t32;
    int reach, mask_words, lazy;
    bool need_suppress;           // the eager track_det_nms pass, for the lists the pick does not maintain
};

// how many steps a chain may take either way from its anchor (vdet/track.py: max_frames boxes in all; 0 = no limit)
int chain_reach(int max_frames, int unbounded) { return max_frames > 0 ? (int)std::ceil((max_frames + 1) / 2.0) - 1 : unbounded; }

// (the scalars first: how many warm chains a call wants depends on them.  reach_unbounded: the caller's kernels' "no max_frames")
TrackWork track_work(vdet_ctx *c, int64_t B, double link_thres, int max_frames, int reach_unbounded)
{
    TrackWork w{};
    w.flags = c->sym_built ? c->gflags.as<uint32_t>() : nullptr;
    if (w.flags && c->index_valid && !c->no_index) w.ix = frame_index_of(c);
    w.filled = B <= kLinkFillMax && w.ix.xbox != nullptr;
    w.link_t32 = thresh_to_f32(link_thres);
    w.reach = chain_reach(max_frames, reach_unbounded);
    w.mask_words = (int)((((size_t)4 * ((B + 31) / 32) + 15) & ~(size_t)15) / 4);
    w.lazy = c->no_lazy ? 0 : 1;
    // (when the host does not know whether every frame is regular -- asynchronous build -- the kernel asks the device)
    w.need_suppress = !w.lazy || !w.flags || !c->all_regular;
    return w;
}

hipError_t reserve_cleared(vdet_ctx *c, DevBuf &b, int byte, size_t bytes)
{
    const hipError_t e = b.reserve(bytes);
    return e != hipSuccess ? e : hipMemsetAsync(b.p, byte, bytes, c->stream);
}

// the scratch of the pick, which every greedy tracker runs: the states, the visited marks and the lazy-list state (t1 | head |
// nkp | pos, [F*C] int32 each), cleared.  The recorded nodes of the call before describe tracks that are about to be replaced
int pick_scratch(vdet_ctx *c, int64_t Ftot, int64_t C, int64_t n_states)
{
    c->nodes_valid = false;
    HIPCHK(c, c->tstate.reserve((size_t)n_states * sizeof(TrackState)));
    HIPCHK(c, reserve_cleared(c, c->visited, 0, (size_t)(Ftot * C)));
    HIPCHK(c, reserve_cleared(c, c->heads, 0, (size_t)(Ftot * C) * 16));
    return VDET_OK;
}

// ... and what the IoU-linking trackers add to it: recorded nodes (0xFF: none), one link memo per call (a link step depends on
// the boxes and link_thres only), and -- with tracks to make -- wm warm chains per state.  (The pixel route needs none of it:
// its tubelet boxes are no proposals and its tracker links nothing.)
int track_scratch(vdet_ctx *c, int64_t Ftot, int64_t B, int64_t C, int T, int wm, int64_t n_states)
{
    const int rc = pick_scratch(c, Ftot, C, n_states);
    if (rc) return rc;
    HIPCHK(c, reserve_cleared(c, c->tracknode, 0xFF, (size_t)std::max<int64_t>(C * T * Ftot, 1) * 4));
    HIPCHK(c, reserve_cleared(c, c->linkmemo, 0, (size_t)2 * Ftot * B * 8));
    HIPCHK(c, reserve_cleared(c, c->linkstats, 0, 16));
    if (T == 0) return VDET_OK;
    HIPCHK(c, c->linkwarm.reserve((size_t)n_states * wm * 4));
    HIPCHK(c, c->linkchains.reserve((size_t)C * wm * Ftot * 5 * 4));
    HIPCHK(c, reserve_cleared(c, c->linknodes, 0xFF, (size_t)C * wm * Ftot * 4));
    return VDET_OK;
}

// the limits of a contiguous [F,B,4] / [F,B,C] volume that every kernel of the volume routes relies on
int check_volume(vdet_ctx *c, const float *d_boxes, int64_t F, int64_t B, int64_t C)
{
    if (B > 32767) return fail(c, VDET_EINVAL, "B = %lld boxes per frame; the limit is 32767", (long long)B);
    if (!fits_upto(0x7FFFFFF0ll, {F, C}) || !fits_upto(0x7FFFFFF0ll, {F, B})) return fail(c, VDET_EINVAL, "volume too large");
    if (((uintptr_t)d_boxes & 15) != 0) return fail(c, VDET_EINVAL, "d_boxes must be 16-byte aligned");
    return VDET_OK;
}

// host-buffer entry points: their group table dies with the call
struct HostGroupsGuard {
    vdet_ctx *c;
    explicit HostGroupsGuard(vdet_ctx *ctx) : c(ctx) {}
    ~HostGroupsGuard() { c->host_groups = nullptr; }
};


// K0 + index + K1(s) + K2 for every batch.
//   volume == false (host-buffer entry points, plan owned by the caller): synchronous, retries once
//     with a larger adjacency pool, clears the device status block (after picking up a failure
//     latched by earlier asynchronous calls).
//   volume == true  (pl == c->vplan): the tables are uploaded once per geometry.  With
//     vdet_set_async and a pool size known from an earlier build there is NO host synchronisation:
//     the status words stay sticky until vdet_sync, which also reports a pool overflow.
int build_graph(vdet_ctx *c, const float4 *d_boxes, NmsPlan &pl, float t32, double thresh, bool volume)
{
    const float one_minus_t = (float)std::max(0.0, 1.0 - (thresh == thresh ? thresh : 0.0));
    const size_t G = pl.groups.size();
    c->host_groups = &pl.groups;
    c->sym_built = false;
    c->gt32 = t32;
    c->wmeta_built = false;
    c->wmeta16_built = false;
    c->nodes_valid = false;      // the adjacency lists the recorded track nodes point into are rewritten
    HIPCHK(c, c->groups.reserve(G * sizeof(GroupDesc)));
    HIPCHK(c, c->tiles.reserve(std::max<size_t>(pl.tiles.size(), 1) * sizeof(TileDesc)));
    HIPCHK(c, c->bits.reserve(std::max<size_t>(pl.bits_words_max, 1) * 8));
    HIPCHK(c, c->rowz.reserve((size_t)pl.ntot * 4));
    HIPCHK(c, c->rowmeta.reserve((size_t)pl.ntot * 8));
    HIPCHK(c, c->groupz.reserve(G * 4));
    HIPCHK(c, c->gflags.reserve(G * 4));
    HIPCHK(c, c->pairs.reserve(std::max<size_t>(pl.pairs.size(), 1) * sizeof(TilePair)));
    HIPCHK(c, c->ditems.reserve(std::max<size_t>(pl.ditems.size(), 1) * sizeof(ListItem)));
    if (!(volume && c->vplan_valid)) {
        if (!pl.pairs.empty())
            HIPCHK(c, hipMemcpyAsync(c->pairs.p, pl.pairs.data(), pl.pairs.size() * sizeof(TilePair),
                                     hipMemcpyHostToDevice, c->stream));
        if (!pl.ditems.empty())
            HIPCHK(c, hipMemcpyAsync(c->ditems.p, pl.ditems.data(), pl.ditems.size() * sizeof(ListItem),
                                     hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->groups.p, pl.groups.data(), G * sizeof(GroupDesc), hipMemcpyHostToDevice, c->stream));
        if (!pl.tiles.empty())
            HIPCHK(c, hipMemcpyAsync(c->tiles.p, pl.tiles.data(), pl.tiles.size() * sizeof(TileDesc),
                                     hipMemcpyHostToDevice, c->stream));
        c->vplan_valid = volume;         // (a host-call plan overwrites the volume tables)
    }
    // direct lists (iou_bits_sym_kernel<true, true>): regular frames of large volumes get a fixed slot per row at the start of
    // the pool, the dynamic part (irregular frames) follows
    auto direct_now = [&]() {
        return c->direct_lists && c->adj_rows && c->wave_transpose && pl.nmax > 384 && sym_threshold_ok(t32) && !c->force_general &&
               (size_t)8 * pl.nmax + 24 * 1024 <= c->max_lds && ((unsigned long long)pl.ntot + 1ull) * c->direct_cap * 2ull + 512ull <= 0xFFFFFFFFull;     // (byte offsets of the entries in 32 bits)
    };
    // (one slot more than rows: where the entries of a column that outgrew its slot are dumped)
    auto fixed_pool = [&]() { return direct_now() ? (unsigned long long)pl.ntot * c->direct_cap + std::max<unsigned long long>(c->direct_cap, 128) : 0ull; };
    unsigned long long min_pool = fixed_pool() + (unsigned long long)pl.ntot * (direct_now() ? 1 : 32);
    const bool async = volume && c->async_enabled && c->pool_hint > 0;
    if (async) {
        const unsigned long long dyn_hint = c->pool_hint > fixed_pool() ? c->pool_hint - fixed_pool() : 0ull;
        const unsigned long long want = std::max(min_pool, fixed_pool() + dyn_hint + dyn_hint / 2);
        if (c->adj.cap < want * 2) HIPCHK(c, c->adj.reserve((size_t)want * 2 + 4096));
    } else {
        // the caller's host vectors must outlive the async copies; also pick up a failure latched by an
        // earlier asynchronous call before the status word is cleared below
        Counters h0;
        HIPCHK(c, hipMemcpyAsync(&h0, c->d_cnt, sizeof h0, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, host_sync(c));
        if (h0.status && !c->latched) c->latched = translate_status(c, h0.status);
        if (h0.eindex && !c->latched) c->latched = fail(c, VDET_EINDEX, "list index out of range");
        if (c->adj.cap < min_pool * 2) HIPCHK(c, c->adj.reserve((size_t)min_pool * 2 + 4096));
    }

    for (int attempt = 0; attempt < 3; ++attempt) {
        const bool direct = direct_now();
        min_pool = fixed_pool() + (unsigned long long)pl.ntot * (direct ? 1 : 32);
        if (!async && c->adj.cap < min_pool * 2) HIPCHK(c, c->adj.reserve((size_t)min_pool * 2 + 4096));
        HIPCHK(c, hipMemsetAsync(c->rowz.p, 0, (size_t)pl.ntot * 4, c->stream));
        HIPCHK(c, hipMemsetAsync(c->rowmeta.p, 0, (size_t)pl.ntot * 8, c->stream));
        HIPCHK(c, hipMemsetAsync(c->groupz.p, 0, G * 4, c->stream));
        if (async) {
            hipLaunchKernelGGL(fold_pool_kernel, dim3(1), dim3(1), 0, c->stream, c->d_cnt);
            HIPCHK(c, hipMemsetAsync((char *)c->d_cnt + kPerBuildOff, 0, sizeof(Counters) - kPerBuildOff, c->stream));
        }
        else HIPCHK(c, hipMemsetAsync(c->d_cnt, 0, sizeof(Counters), c->stream));
        c->direct_ntot = direct ? pl.ntot : 0;
        c->direct_fixed = fixed_pool();
        if (direct) hipLaunchKernelGGL(pool_start_kernel, dim3(1), dim3(1), 0, c->stream, &c->d_cnt->pool_used, fixed_pool());
        const int pool_bits = async ? (kStPool | kStPoolAsync) : kStPool;
        const unsigned long long pool_cap = (c->adj.cap - 2048) / 2;     // (the packed walk reads up to 256 B past a list)
        // fast symmetric kernel for regular frames needs a threshold its divide-free test is exact for (sym_threshold_ok)
        // ... and the x1 index, whose sort must fit the LDS (8 B per box + tables)
        const bool use_sym = sym_threshold_ok(t32) && !c->force_general &&
                             (size_t)8 * pl.nmax + 24 * 1024 <= c->max_lds;
        c->sym_built = use_sym;
        c->wmeta_built = use_sym;
        if (c->wmeta_built) HIPCHK(c, c->wmeta.reserve((size_t)pl.ntot * sizeof(WalkMeta)));
        if (c->wmeta_built && c->adj_rows && pl.nmax > 384) HIPCHK(c, c->wmeta16.reserve((size_t)pl.ntot * sizeof(uint4)));
        if (use_sym) {
            {
                StageTimer tm(c, ST_OTHER);
                hipLaunchKernelGGL(frame_flags_kernel, dim3((unsigned)G), dim3(256), 0, c->stream, d_boxes,
                                   c->groups.as<GroupDesc>(), c->gflags.as<uint32_t>(), &c->d_cnt->irregular);
            }
            // (the index cache is keyed on the boxes pointer: never valid for the context's own scratch)
            if (!volume) c->index_valid = false;
            const int rci = build_frame_index(c, d_boxes, pl.ntot, (int64_t)G, pl.nmax);
            if (rci) return rci;
            // which 64 x 64 blocks of the predicate matrix can hold a set bit (K1s writes, K2 reads only those)
            HIPCHK(c, c->reachtab.reserve((size_t)(pl.ntot / 64 + (int64_t)G + 2) * sizeof(float2)));
            {
                StageTimer tm(c, ST_OTHER);
                hipLaunchKernelGGL(reach_table_kernel, dim3((unsigned)G), dim3(256), 0, c->stream, c->xbox.as<float4>(),
                                   c->groups.as<GroupDesc>(), c->gflags.as<uint32_t>(), one_minus_t, c->reachtab.as<float2>());
                if (direct) {      // the tiles' rows by width: one quartile per wave of the predicate kernel
                    HIPCHK(c, c->rowperm.reserve((size_t)pl.ntot * 2 + 1024));
                    HIPCHK(c, c->qreach.reserve((size_t)(pl.ntot / 256 + (int64_t)G + 2) * 4 * sizeof(float)));
                    hipLaunchKernelGGL(row_classes_kernel, dim3((unsigned)G, (unsigned)((pl.nmax + 255) / 256)), dim3(256), 0, c->stream,
                                       c->xbox.as<float4>(), c->groups.as<GroupDesc>(), c->gflags.as<uint32_t>(), one_minus_t,
                                       c->rowperm.as<uint16_t>(), c->qreach.as<float>());
                }
            }
        } else {
            c->index_valid = false;      // gflags / the x-index describe some earlier boxes
        }
        if (direct && !pl.ditems.empty()) {
            // ONE launch for every regular frame of the plan (no bit matrix: nothing ties the launch to the batches below): a
            // work item is a wave that runs 90-250 us, and four launches of two rounds of items each were a quarter tail
            StageTimer tm(c, ST_IOU_BITS);
            GraphListsParams gp;
            gp.xbox = c->xbox.as<float4>(); gp.xord = c->xord.as<uint16_t>(); gp.groups = c->groups.as<GroupDesc>();
            gp.group_flags = c->gflags.as<uint32_t>(); gp.items = c->ditems.as<ListItem>(); gp.nitems = (int)pl.ditems.size();
            gp.t32 = t32; gp.hg = half_gap(t32); gp.one_minus_t = one_minus_t; gp.row_deg = c->rowz.as<uint32_t>(); gp.reach_table = c->reachtab.as<float2>();
            gp.rowperm = c->rowperm.as<uint16_t>(); gp.qreach = c->qreach.as<float>(); gp.adj = c->adj.as<uint16_t>();
            gp.slot_cap = c->direct_cap; gp.status = &c->d_cnt->status; gp.over_bits = pool_bits | kStDirect;
            gp.trash_off = (uint32_t)((unsigned long long)pl.ntot * c->direct_cap * 2ull);      // (the spare slot behind the rows')
            hipLaunchKernelGGL(graph_lists_kernel, dim3((gp.nitems + 7) & ~7), dim3(64), 0, c->stream, gp);
        }
        for (size_t bi = 0; bi < pl.batch_tiles.size(); ++bi) {
            const auto bt = pl.batch_tiles[bi];
            const auto bp = pl.batch_pairs[bi];
            const int nt = bt.second - bt.first;
            if (nt <= 0) continue;
            uint64_t *bits_b = c->bits.as<uint64_t>();
            if (use_sym && !direct && bp.second > bp.first) {       // (the direct lists: one launch for all frames, above)
                StageTimer tm(c, ST_IOU_BITS);
                if (c->wave_transpose)
                    hipLaunchKernelGGL(iou_bits_sym_kernel<true>, dim3(bp.second - bp.first), dim3(256), 0, c->stream,
                                       c->xbox.as<float4>(), c->groups.as<GroupDesc>(), c->gflags.as<uint32_t>(),
                                       c->pairs.as<TilePair>() + bp.first, t32, half_gap(t32), one_minus_t, bits_b, c->rowz.as<uint32_t>(),
                                       c->reachtab.as<float2>());
                else
                    hipLaunchKernelGGL(iou_bits_sym_kernel<false>, dim3(bp.second - bp.first), dim3(256), 0, c->stream,
                                       c->xbox.as<float4>(), c->groups.as<GroupDesc>(), c->gflags.as<uint32_t>(),
                                       c->pairs.as<TilePair>() + bp.first, t32, half_gap(t32), one_minus_t, bits_b, c->rowz.as<uint32_t>(),
                                       c->reachtab.as<float2>());
            }
            // enough column splits to fill the chip when there are few row tiles
            int splits = 1;
            if (nt < 4 * c->n_cu) {
                int wmax = 1;
                for (int t = bt.first; t < bt.second; ++t)
                    wmax = std::max(wmax, (pl.groups[pl.tiles[t].group].nbox + 63) / 64);
                splits = std::min((4 * c->n_cu + nt - 1) / nt, (wmax + 3) / 4);
                splits = std::max(1, std::min(splits, 65535));
            }
            {
                StageTimer tm(c, ST_IOU_GEN);
                hipLaunchKernelGGL(iou_bits_kernel, dim3(nt, splits), dim3(256), 0, c->stream, d_boxes,
                                   c->groups.as<GroupDesc>(), c->tiles.as<TileDesc>() + bt.first, t32,
                                   bits_b, c->rowz.as<uint32_t>(), c->groupz.as<uint32_t>(),
                                   use_sym ? c->gflags.as<uint32_t>() : (const uint32_t *)nullptr);
            }
            {
                StageTimer tm(c, ST_ADJ);
                const bool k2_tile = pl.nmax <= 384;      // small frames: one block per tile
                const bool rows_path = use_sym && c->adj_rows && !k2_tile;
                hipLaunchKernelGGL(k2_tile ? adj_build_kernel<kRowsPerTile> : adj_build_kernel<kAdjRows>, dim3(k2_tile ? nt : 2 * nt),
                                   dim3(k2_tile ? kRowsPerTile : kAdjRows), 0, c->stream, d_boxes,
                                   c->groups.as<GroupDesc>(), c->tiles.as<TileDesc>() + bt.first,
                                   bits_b, c->rowz.as<uint32_t>(), c->rowmeta.as<uint2>(),
                                   c->adj.as<uint16_t>(), &c->d_cnt->pool_used, pool_cap,
                                   &c->d_cnt->status, use_sym ? c->gflags.as<uint32_t>() : (const uint32_t *)nullptr,
                                   use_sym ? frame_index_of(c) : FrameIndex{}, one_minus_t,
                                   async ? (kStPool | kStPoolAsync) : kStPool,
                                   c->wmeta_built ? c->wmeta.as<WalkMeta>() : (WalkMeta *)nullptr,
                                   use_sym ? c->reachtab.as<float2>() : (const float2 *)nullptr, rows_path ? 1 : 0);
                // regular groups of large frames: one workgroup per 64-row strip, half a wave per row (adjrows_kernels.hpp)
                if (rows_path && direct) {
                    // (one launch for all tiles, behind the first batch: the lists of every regular frame are complete by then)
                    if (bi == 0)
                    hipLaunchKernelGGL(adj_finish_kernel, dim3((unsigned)pl.tiles.size()), dim3(256), 0, c->stream, c->groups.as<GroupDesc>(),
                                       c->tiles.as<TileDesc>(), c->rowz.as<uint32_t>(), c->rowmeta.as<uint2>(),
                                       c->adj.as<uint16_t>(), c->direct_cap, &c->d_cnt->status, c->gflags.as<uint32_t>(),
                                       c->xbox.as<float4>(), c->xord.as<uint16_t>(), pool_bits | kStDirect,
                                       c->wmeta_built ? c->wmeta.as<WalkMeta>() : (WalkMeta *)nullptr,
                                       c->wmeta_built ? c->wmeta16.as<uint4>() : (uint4 *)nullptr);
                    c->wmeta16_built = c->wmeta_built;
                } else if (rows_path) {
                    // every strip's slab offset first (two small launches instead of an atomic per strip on one address)
                    HIPCHK(c, c->striptot.reserve((size_t)4 * nt * 4));
                    HIPCHK(c, c->stripoff.reserve((size_t)4 * nt * 8));
                    hipLaunchKernelGGL(strip_totals_kernel, dim3(nt), dim3(256), 0, c->stream, c->groups.as<GroupDesc>(),
                                       c->tiles.as<TileDesc>() + bt.first, 4 * nt, c->rowz.as<uint32_t>(), c->gflags.as<uint32_t>(),
                                       c->striptot.as<uint32_t>());
                    hipLaunchKernelGGL(strip_scan_kernel, dim3(1), dim3(1024), 0, c->stream, c->striptot.as<uint32_t>(), 4 * nt,
                                       c->stripoff.as<unsigned long long>(), &c->d_cnt->pool_used);
                    hipLaunchKernelGGL(adj_rows_kernel, dim3(4 * nt), dim3(256), 0, c->stream, c->groups.as<GroupDesc>(),
                                       c->tiles.as<TileDesc>() + bt.first, bits_b, c->rowz.as<uint32_t>(), c->rowmeta.as<uint2>(),
                                       c->adj.as<uint16_t>(), c->stripoff.as<unsigned long long>(), pool_cap, &c->d_cnt->status, c->gflags.as<uint32_t>(),
                                       c->xbox.as<float4>(), c->xord.as<uint16_t>(), async ? (kStPool | kStPoolAsync) : kStPool,
                                       c->wmeta_built ? c->wmeta.as<WalkMeta>() : (WalkMeta *)nullptr, c->reachtab.as<float2>(),
                                       c->wmeta_built ? c->wmeta16.as<uint4>() : (uint4 *)nullptr);
                    c->wmeta16_built = c->wmeta_built;
                }
            }
        }
        HIPCHK(c, hipGetLastError());
        if (async) {
            c->all_regular = false;      // not known on the host: the tracking loop asks the device (n_irregular)
            return VDET_OK;
        }
        Counters h;
        HIPCHK(c, hipMemcpyAsync(&h, c->d_cnt, sizeof h, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, host_sync(c));
        c->all_regular = use_sym && h.irregular == 0;
        if (!(h.status & kStPool)) {
            c->pool_hint = std::max(c->pool_hint, h.pool_used);
            return VDET_OK;
        }
        if (h.status & kStDirect) {     // a row with more neighbours than a direct slot holds: through the bit matrix from now on
            c->direct_lists = false;
            continue;
        }
        if (h.pool_used > 0xFFFFFFFFull) return fail(c, VDET_ENOMEM, "suppression graph has more than 2^32 edges");
        if (attempt == 2) break;
        HIPCHK(c, c->adj.reserve((size_t)h.pool_used * 2 + 4096));
    }
    return fail(c, VDET_EHIP, "internal: adjacency pool overflow after regrow");
}

// K3 + K4 for P problems.  d_order / d_ncand / keep buffers are caller-provided device pointers.
struct SortWalkArgs {
    bool sort_only = false;       // tracking: only the per-problem lists are wanted
    bool walk_only = false;       // the lists of a previous call are still valid
    uint16_t *order_out = nullptr;   // default: ctx scratch (c->order / c->ncand)
    int32_t *ncand_out = nullptr;
    const uint16_t *order_in = nullptr;   // walk_only: the caller's own lists instead of the context's
    const int32_t *ncand_in = nullptr;
    int mode, P, B, C;
    const float *scores;
    const uint32_t *keys;
    const uint8_t *excl;
    int use_thr;
    float thr;
    int topk = 0;
    int32_t *nover_out = nullptr; // candidates of every list before the topk cut
    int32_t *keep_idx;
    int32_t *keep_cnt;
    int64_t cap;
};

// an [F,B,C] score volume through the transposed keys: only the descending lists per (frame, class) ...
SortWalkArgs volume_sort_args(int64_t F, int64_t B, int64_t C, const float *d_scores)
{
    SortWalkArgs a{};
    a.sort_only = true;
    a.mode = 0; a.P = (int)(F * C); a.B = (int)B; a.C = (int)C;
    a.scores = d_scores;
    return a;
}

// ... and only the walk over them (the lists stay in place)
SortWalkArgs volume_walk_args(int64_t F, int64_t B, int64_t C, const float *d_scores, int32_t *keep_idx, int32_t *keep_cnt, int64_t cap)
{
    SortWalkArgs a = volume_sort_args(F, B, C, d_scores);
    a.sort_only = false;
    a.walk_only = true;
    a.keep_idx = keep_idx; a.keep_cnt = keep_cnt; a.cap = cap;
    return a;
}

int sort_comp_desc(vdet_ctx *c, uint32_t n);

int launch_sort_walk(vdet_ctx *c, const SortWalkArgs &a, int nmax, int64_t order_elems)
{
    if (a.P <= 0) return VDET_OK;
    auto r16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    if (!a.order_out) {
        HIPCHK(c, c->order.reserve((size_t)std::max<int64_t>(order_elems, 1) * 2));
        HIPCHK(c, c->ncand.reserve((size_t)a.P * 4));
    }
    const int block = nmax > 1024 ? 1024 : 256;
    const int nw = block / 64;
    const int nchunks = (std::max(nmax, 1) + 63) / 64;
    const int need_cpw = (nchunks + nw - 1) / nw;
    // instantiated (BLOCK, CPW) pairs; CPW = chunks of 64 keys per wave
    struct Variant { int block, cpw; const void *fn[2]; const void *fn_list[2]; };   // [0]: ballot match, [1]: atomic rank
#define VDET_SV(BL, CP) {BL, CP, {reinterpret_cast<const void *>(sort_kernel<BL, CP, false>), reinterpret_cast<const void *>(sort_kernel<BL, CP, true>)}, \
                         {reinterpret_cast<const void *>(sort_list_kernel<BL, CP, false>), reinterpret_cast<const void *>(sort_list_kernel<BL, CP, true>)}}
    static const Variant variants[] = {VDET_SV(256, 1), VDET_SV(256, 2), VDET_SV(256, 4), VDET_SV(1024, 2), VDET_SV(1024, 4),
                                       VDET_SV(1024, 6), VDET_SV(1024, 8), VDET_SV(1024, 10), VDET_SV(1024, 12),
                                       VDET_SV(1024, 16), VDET_SV(1024, 18)};
#undef VDET_SV
    if (!c->sort_attr_set) {
        size_t stat = 0;
        std::vector<const void *> fns;
        for (const Variant &v : variants) { fns.push_back(v.fn[0]); fns.push_back(v.fn[1]); fns.push_back(v.fn_list[0]); fns.push_back(v.fn_list[1]); }
        fns.push_back(reinterpret_cast<const void *>(walk_kernel));
        for (const void *fn : {reinterpret_cast<const void *>(binsort_kernel<8, false>), reinterpret_cast<const void *>(binsort_kernel<8, true>),
                               reinterpret_cast<const void *>(binsort_kernel<20, false>), reinterpret_cast<const void *>(binsort_kernel<20, true>),
                               reinterpret_cast<const void *>(binsort_kernel<36, false>), reinterpret_cast<const void *>(binsort_kernel<36, true>)})
            fns.push_back(fn);
        for (const void *fn : fns) {
            hipFuncAttributes fa;
            HIPCHK(c, hipFuncGetAttributes(&fa, fn));
            stat = std::max(stat, (size_t)fa.sharedSizeBytes);
        }
        c->dyn_lds_max = c->max_lds - r16(stat);
        for (const void *fn : fns)
            HIPCHK(c, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->dyn_lds_max));
        c->sort_attr_set = true;
    }
    const Variant *var = nullptr;
    for (const Variant &v : variants)
        if (v.block == block && v.cpw >= need_cpw) { var = &v; break; }
    SortParams sp{};
    sp.mode = a.mode; sp.P = a.P; sp.B = a.B; sp.C = a.C;
    sp.scores = a.scores; sp.keys = a.keys; sp.excl = a.excl; sp.use_thr = a.use_thr; sp.thr = a.thr;
    if (a.mode == 0 && !a.keys && !a.walk_only) {
        // class-innermost volume: one coalesced transpose to [F,C,B] keys, then the sort reads rows
        const int64_t F = a.P / a.C;
        const bool have_keys = c->cache_enabled && c->keys_valid && c->keysrc.scores == a.scores && c->keysrc.F == F &&
                               c->keysrc.B == a.B && c->keysrc.C == a.C && c->keysrc.use_thr == (a.use_thr ? 1 : 0) &&
                               (!a.use_thr || c->keysrc.thr == a.thr);     // left there by vdet_volume_pass
        if (!have_keys) c->keys_valid = false;
        HIPCHK(c, c->tkeys.reserve((size_t)a.P * a.B * 4));
        if (!have_keys) {
            StageTimer tm(c, ST_TRANSPOSE);
            hipLaunchKernelGGL(transpose_keys_kernel, dim3((a.B + 63) / 64, (a.C + 63) / 64, (unsigned)F), dim3(256), 0,
                               c->stream, a.scores, c->tkeys.as<uint32_t>(), a.B, a.C, a.use_thr, a.thr);
        }
        HIPCHK(c, hipGetLastError());
        sp.mode = 3;             // keys laid out [P,B] (decode like mode 1)
        sp.keys = c->tkeys.as<uint32_t>();
        sp.scores = nullptr;
        sp.use_thr = 0;
    }
    sp.groups = c->groups.as<GroupDesc>();
    sp.order = a.order_out ? a.order_out : c->order.as<uint16_t>();
    sp.ncand = a.order_out ? a.ncand_out : c->ncand.as<int32_t>();
    sp.topk = a.topk;
    sp.nover = a.nover_out;
    const size_t keysB = r16((size_t)2 * std::max(nmax, 1));     // 16 key bits at a time (see sort_kernel)
    const size_t idxB = r16((size_t)2 * std::max(nmax, 1));
    sp.lds_idxa_off = (int)keysB;
    sp.lds_idxb_off = (int)(keysB + idxB);
    sp.lds_base_off = (int)(keysB + 2 * idxB);
    const size_t lds = keysB + 2 * idxB + (size_t)4 * (nw * 256 + 256 + 4);
    const bool big = !var || lds > c->dyn_lds_max;
    if (big && a.mode != 2)
        return fail(c, VDET_EINVAL, "a frame with %d boxes needs %zu B of LDS for the in-LDS sort; the limit is %zu B "
                                    "(about 18000 boxes per frame)", nmax, lds, c->dyn_lds_max);
    if (big && !a.walk_only) {
        // flat groups (host-buffer entry points) beyond the LDS limit: one global bitonic sort per
        // group.  Slow path for rare, very large single problems (<= 32767 boxes).
        if (!c->host_groups || (int)c->host_groups->size() != a.P) return fail(c, VDET_EINVAL, "internal: group table missing");
        HIPCHK(c, hipMemsetAsync(sp.ncand, 0, (size_t)a.P * 4, c->stream));
        StageTimer tm(c, ST_SORTK);
        for (int g = 0; g < a.P; ++g) {
            const GroupDesc &gd = (*c->host_groups)[(size_t)g];
            const int n = gd.nbox;
            if (n <= 0) continue;
            const uint32_t n2 = pow2ceil((uint32_t)n);
            HIPCHK(c, c->comp.reserve((size_t)n2 * 8));
            hipLaunchKernelGGL(fill_comp_kernel, dim3((n2 + 255) / 256), dim3(256), 0, c->stream, a.scores, a.keys, a.excl,
                               a.use_thr, a.thr, (int64_t)gd.box_off, n, n2, c->comp.as<unsigned long long>(), sp.ncand + g);
            const int rc = sort_comp_desc(c, n2);
            if (rc) return rc;
            hipLaunchKernelGGL(comp_to_order_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream,
                               c->comp.as<unsigned long long>(), n, sp.order + gd.box_off);
        }
        HIPCHK(c, hipGetLastError());
    } else if (!a.walk_only) {
        // volumes of untied scores: the equalised counting sort (binsort_kernels.hpp); what it can not spread -- decided per
        // problem on the device -- lands on a list the LSD kernel works off afterwards (normally empty)
        const int bin_cpw = nmax <= 4096 ? 8 : nmax <= 10240 ? 20 : 36;      // keys per thread, 512 threads
        const size_t bin_lds = binsort_lds_bytes(std::max(nmax, 1), bin_cpw);
        // (threshold / top-k / exclusion lists change ncand: those go to the LSD kernel; a NaN inside an otherwise plain list is
        //  caught per list on the device, binsort_kernels.hpp phase 3)
        const bool use_bin = c->binsort && (sp.mode == 1 || sp.mode == 3) && a.topk == 0 && !a.use_thr && !a.excl && block == 1024 &&
                             nmax <= 512 * bin_cpw && bin_lds + 4096 <= c->dyn_lds_max;
        // frames of at most 384 boxes: one WAVE per list (small_kernels.hpp: the same stable LSD passes without a workgroup)
        const bool use_small = c->small_lists && c->atomic_rank && a.mode != 2 && nmax <= kSmallMax && a.topk == 0 && !a.excl && !a.nover_out;
        StageTimer tm(c, ST_SORTK);
        if (a.mode != 2) c->last_sort_binned = use_bin && !use_small;
        if (use_small) {
            const int kpl = std::max(1, (nmax + 63) / 64);
            const int grid = (((a.P + 3) / 4) + 7) & ~7;
            void *args[] = {&sp};
            const void *fn = kpl == 1 ? reinterpret_cast<const void *>(small_sort_kernel<1>) : kpl == 2 ? reinterpret_cast<const void *>(small_sort_kernel<2>)
                           : kpl == 3 ? reinterpret_cast<const void *>(small_sort_kernel<3>) : kpl == 4 ? reinterpret_cast<const void *>(small_sort_kernel<4>)
                           : kpl == 5 ? reinterpret_cast<const void *>(small_sort_kernel<5>) : reinterpret_cast<const void *>(small_sort_kernel<6>);
            HIPCHK(c, hipLaunchKernel(fn, dim3(grid), dim3(256), args, 0, c->stream));
        } else if (use_bin) {
            HIPCHK(c, c->sortctl.reserve(sizeof(BinSortCtl) + (size_t)a.P * 4));
            HIPCHK(c, hipMemsetAsync(c->sortctl.p, 0, sizeof(BinSortCtl), c->stream));
            BinSortParams bp{};
            const bool floats = sp.keys == nullptr;
            bp.raw = floats ? reinterpret_cast<const uint32_t *>(sp.scores) : sp.keys;
            bp.P = a.P; bp.N = a.B;
            bp.order = sp.order; bp.ncand = sp.ncand;
            bp.ctl = c->sortctl.as<BinSortCtl>();
            bp.fail_list = reinterpret_cast<int32_t *>(c->sortctl.as<char>() + sizeof(BinSortCtl));
            const int per_cu = std::max<int>(1, (int)(c->max_lds / (bin_lds + 4096)));
            bp.inherit = c->binsort_inherit ? 1 : 0;
            const int full = std::min(a.P, per_cu * c->n_cu);
            const int grid = c->binsort_grid > 0 ? std::min(full, c->binsort_grid) : full;
#define VDET_BSK(CP) (floats ? reinterpret_cast<const void *>(binsort_kernel<CP, true>) : reinterpret_cast<const void *>(binsort_kernel<CP, false>))
            const void *bfn = bin_cpw == 8 ? VDET_BSK(8) : bin_cpw == 20 ? VDET_BSK(20) : VDET_BSK(36);
#undef VDET_BSK
            void *bargs[] = {&bp};
            HIPCHK(c, hipLaunchKernel(bfn, dim3(grid), dim3(512), bargs, bin_lds, c->stream));
            const int32_t *fl = bp.fail_list;
            const int *fc = &bp.ctl->nfail;
            void *largs[] = {&sp, (void *)&fl, (void *)&fc};
            StageTimer tm2(c, ST_SORTFB);
            HIPCHK(c, hipLaunchKernel(var->fn_list[c->atomic_rank ? 1 : 0], dim3(std::min(a.P, 2 * c->n_cu)), dim3(block), largs, lds, c->stream));
        } else {
            const int grid = (a.P + 7) & ~7;
            void *args[] = {&sp};
            HIPCHK(c, hipLaunchKernel(var->fn[c->atomic_rank ? 1 : 0], dim3(grid), dim3(block), args, lds, c->stream));
        }
    }
    HIPCHK(c, hipGetLastError());
    if (a.sort_only) return VDET_OK;
    WalkParams wp{};
    wp.mode = a.mode; wp.P = a.P; wp.B = a.B; wp.C = a.C;
    wp.groups = c->groups.as<GroupDesc>();
    wp.order = a.order_in ? a.order_in : c->order.as<uint16_t>();
    wp.ncand = a.order_in ? a.ncand_in : c->ncand.as<int32_t>();
    wp.row_meta = c->rowmeta.as<uint2>();
    wp.adj = c->adj.as<uint16_t>();
    wp.group_z = c->groupz.as<uint32_t>();
    wp.keep_idx = a.keep_idx;
    wp.keep_cnt = a.keep_cnt;
    wp.cap = a.cap;
    wp.status = &c->d_cnt->status;
    wp.mask_words = (int)(r16((size_t)4 * ((std::max(nmax, 1) + 31) / 32)) / 4);
    wp.group_flags = c->sym_built ? c->gflags.as<uint32_t>() : nullptr;   // frames whose graph is symmetric
    wp.packed = (wp.group_flags && c->wmeta_built) ? 1 : 0;               // regular frames: eight candidates per pass
    wp.wave_words = wp.mask_words + (wp.packed ? 8 * kPackRing : 0);      // + the ring of alive candidates
    wp.wmeta = c->wmeta.as<WalkMeta>();
    wp.t32 = c->gt32;
    wp.wmeta16 = (wp.packed && c->wmeta16_built) ? c->wmeta16.as<uint4>() : nullptr;
    wp.adj32 = c->adj.cap <= 0xFFFFFF00ull ? 1 : 0;
    wp.wide_nsw = wp.packed ? c->walk_wide_nsw : 0;
    if (wp.packed) wp.wave_words += kWideStage;                           // + the wide filter's staging behind the ring
    c->last_walk_wide = wp.wide_nsw > 0;
    if (wp.wide_nsw > 0) {
        HIPCHK(c, c->walkstats.reserve(sizeof(uint32_t) * 2 * kWideStatSlots));
        HIPCHK(c, hipMemsetAsync(c->walkstats.p, 0, sizeof(uint32_t) * 2 * kWideStatSlots, c->stream));
        wp.wide_stats = c->walkstats.as<uint32_t>();
    }
    // frames of at most 384 boxes: one LANE per list, the frames' rows in LDS (small_kernels.hpp); the lists of irregular frames
    // are left to the general walk (walk_rest_kernel: normally nothing)
    const bool small_walk = c->small_lists && a.mode != 2 && nmax <= kSmallMax && wp.group_flags && a.C > 0 && a.P % a.C == 0;
    if (small_walk) {
        const int G = a.P / a.C;
        const int nq = nmax <= 128 ? 1 : nmax <= 256 ? 2 : 3;
        const int nm = std::max(nmax, 1);
        const size_t row_bytes = (size_t)nm * 4 * nq * 4;
        const int fpw = a.C > 32 ? 1 : (int)std::max<size_t>(1, std::min<size_t>((size_t)(64 / a.C), (size_t)(44 * 1024) / row_bytes));
        const size_t lds_bytes = (size_t)fpw * row_bytes;
        // a list's candidates four per 8-byte load: rows of B % 4 == 0 entries from an 8-byte aligned base (the caller's lists of
        // vdet_nms_volume_ordered may sit anywhere)
        const int vec4 = (a.B % 4 == 0 && ((uintptr_t)wp.order & 7) == 0) ? 1 : 0;
        const int grid = (G + fpw - 1) / fpw;
        StageTimer tm(c, ST_WALK);
#define VDET_SMALLW(NQ_, V_) hipLaunchKernelGGL((small_walk_kernel<NQ_, V_>), dim3(grid), dim3(64), lds_bytes, c->stream, wp, G, fpw, nm)
        if (vec4) { if (nq == 1) VDET_SMALLW(1, true); else if (nq == 2) VDET_SMALLW(2, true); else VDET_SMALLW(3, true); }
        else { if (nq == 1) VDET_SMALLW(1, false); else if (nq == 2) VDET_SMALLW(2, false); else VDET_SMALLW(3, false); }
#undef VDET_SMALLW
        if (!c->all_regular)      // (asynchronous build: not known on the host -- the kernel looks at the frames' flags)
            hipLaunchKernelGGL(walk_rest_kernel, dim3(std::min(G, 4 * c->n_cu)), dim3(256), (size_t)wp.wave_words * 4 * 4, c->stream, wp, G);
    } else {
        const int nblk = (((a.P + 3) / 4) + 7) & ~7;
        StageTimer tm(c, ST_WALK);
        hipLaunchKernelGGL(walk_kernel, dim3(nblk), dim3(256), (size_t)wp.wave_words * 4 * 4, c->stream, wp);
    }
    HIPCHK(c, hipGetLastError());
    return VDET_OK;
}

// ---- the front half of the greedy volume trackers (vdet_nms_track_volume, vdet_track_volume_pixels; its first step also
// opens vdet_video_batch).  In this order: volume_lists, track_work, the caller's scratch and warm-up, track_begin, greedy_args.
// The suppression graph of the boxes and the descending lists per (frame, class), always through the transposed keys (the pick
// needs them).  reuse (as ensure_volume_graph's): resident ones that match may serve.  lists_valid is left alone: the link
// route still walks the NMS survivors over the lists before track_begin gives them to the tracker.
int volume_lists(vdet_ctx *c, const float *d_boxes, const float *d_scores, int64_t F, int64_t B, int64_t C, double nms_thres, bool reuse)
{
    bool same_geo = false;
    const int rc = ensure_volume_graph(c, d_boxes, F, B, nms_thres, reuse, &same_geo);
    if (rc || (same_geo && lists_match(c, ListsKey{d_scores, C, VDET_LAYOUT_FBC, 0, 0.f, 0}, F, B))) return rc;
    return launch_sort_walk(c, volume_sort_args(F, B, C, d_scores), (int)B, F * C * B);
}

// The lists are the tracker's from here (it compacts them in place): every class at "no track yet", ntracks = 0.  With nothing
// to track the caller returns, and a launch error of the calls so far is reported by THIS call.
int track_begin(vdet_ctx *c, int64_t C, int max_tracks, int32_t *d_ntracks)
{
    c->lists_valid = false;
    hipLaunchKernelGGL(track_init_kernel, dim3((unsigned)((C + 63) / 64)), dim3(64), 0, c->stream, c->tstate.as<TrackState>(), (int)C);
    HIPCHK(c, hipMemsetAsync(d_ntracks, 0, (size_t)C * 4, c->stream));
    if (max_tracks == 0) HIPCHK(c, hipGetLastError());
    return VDET_OK;
}

// What pick, lazy lists and the eager pass read, from the context's buffers (graph: build_graph; lists: volume_lists; scratch:
// pick_scratch), the TrackWork and the caller's pointers.  A tracker that links adds its own fields of LoopArgs.
struct GreedyArgs { SuppressParams sp; LazyLists lz; LoopArgs la; };

GreedyArgs greedy_args(vdet_ctx *c, const TrackWork &w, const float *d_boxes, const float *d_scores, int64_t F, int64_t B, int64_t C,
                       double nms_thres, double thres, int max_tracks, float *d_tracks, float *d_anchors, int32_t *d_ntracks)
{
    GreedyArgs g{};
    SuppressParams &sp = g.sp;
    sp.boxes = reinterpret_cast<const float4 *>(d_boxes);
    sp.F = (int)F; sp.B = (int)B; sp.C = (int)C; sp.max_tracks = max_tracks;
    sp.groups = c->groups.as<GroupDesc>();
    sp.row_meta = c->rowmeta.as<uint2>();
    sp.adj = c->adj.as<uint16_t>();
    sp.group_z = c->groupz.as<uint32_t>();
    sp.group_flags = w.flags; sp.ix = w.ix;
    sp.thres = nms_thres;
    sp.lists = c->order.as<uint16_t>();
    sp.cnt = c->ncand.as<int32_t>();
    sp.visited = c->visited.as<uint8_t>();
    sp.st = c->tstate.as<TrackState>();
    sp.tracks = d_tracks;
    sp.t32 = thresh_to_f32(nms_thres);
    sp.status = &c->d_cnt->status;
    sp.mask_words = w.mask_words; sp.lazy = w.lazy;
    sp.n_irregular = &c->d_cnt->irregular;
    LazyLists &lz = g.lz;
    lz.boxes = sp.boxes; lz.tracks = d_tracks; lz.t32 = sp.t32;
    lz.t1 = c->heads.as<int32_t>(); lz.head = lz.t1 + F * C; lz.nkp = lz.head + F * C; lz.pos = lz.nkp + F * C;
    lz.group_flags = sp.lazy ? sp.group_flags : nullptr;
    LoopArgs &la = g.la;
    la.keys = c->tkeys.as<uint32_t>(); la.lists = sp.lists; la.cnt = sp.cnt;
    la.scores = d_scores; la.thres = thres; la.anchors = d_anchors;
    la.ntracks_out = d_ntracks;
    la.need_suppress = w.need_suppress ? 1 : 0;
    return g;
}

// the checks of the pixel tracker's settings, shared by vdet_track_pixels[_scaled] and vdet_track_volume_pixels[_scaled]
int pix_settings_check(vdet_ctx *c, int64_t H, int64_t W, int S, int R, double min_conf, int max_frames, int step, const PixScaleArgs *sc)
{
    if (H > 32767 || W > 32767) return fail(c, VDET_EINVAL, "images of at most 32767 rows and columns");
    if (S < 4 || S > kPixMaxS || S % 4) return fail(c, VDET_EINVAL, "grid = %d; a multiple of 4 in 4 .. %d", S, kPixMaxS);
    if (R < 1 || R > kPixMaxR) return fail(c, VDET_EINVAL, "radius = %d; 1 .. %d", R, kPixMaxR);
    if (step < 1 || max_frames < 0) return fail(c, VDET_EINVAL, "step must be >= 1 and max_frames >= 0");
    if (!std::isfinite(min_conf)) return fail(c, VDET_EINVAL, "min_conf must be finite");
    if (!sc) return VDET_OK;
    if (sc->ns < 0 || sc->ns > kPixMaxScales) return fail(c, VDET_EINVAL, "scales = %d; 0 .. %d", sc->ns, kPixMaxScales);
    if (sc->p < 1 || sc->p > kPixMaxScaleStep) return fail(c, VDET_EINVAL, "scale_step = %d; 1 .. %d", sc->p, kPixMaxScaleStep);
    if (sc->q < 0 || sc->q > kPixMaxScalePenalty) return fail(c, VDET_EINVAL, "scale_penalty = %d; 0 .. %d", sc->q, kPixMaxScalePenalty);
    return VDET_OK;
}

int sort_groups_by_keys(vdet_ctx *c, int G, int nmax, int64_t ntot)
{
    SortWalkArgs a{};
    a.sort_only = true;
    a.mode = 2; a.P = G;
    a.keys = c->xkeys.as<uint32_t>();
    a.order_out = c->xord.as<uint16_t>();
    a.ncand_out = c->xncand.as<int32_t>();
    const bool st = c->timing;
    c->timing = false;                       // keep the per-(frame,class) sort stage clean
    const int rc = launch_sort_walk(c, a, nmax, ntot);
    c->timing = st;
    return rc;
}

// descending sort of n composites held in c->comp (zero padded to a power of two)
int sort_comp_desc(vdet_ctx *c, uint32_t n)
{
    if (n <= 1) return VDET_OK;
    const uint32_t n2 = pow2ceil(n);
    unsigned long long *d = c->comp.as<unsigned long long>();
    StageTimer tm(c, ST_SORT);
    const uint32_t nb = (n2 + 2047) / 2048;
    hipLaunchKernelGGL(bitonic_lds_kernel, dim3(nb), dim3(1024), 0, c->stream, d, n2, 2u, std::min(n2, 2048u));
    for (uint32_t k = 4096; k <= n2 && k; k <<= 1) {
        for (uint32_t j = k >> 1; j >= 2048; j >>= 1)
            hipLaunchKernelGGL(bitonic_global_step, dim3((n2 + 255) / 256), dim3(256), 0, c->stream, d, n2, j, k);
        hipLaunchKernelGGL(bitonic_lds_kernel, dim3(nb), dim3(1024), 0, c->stream, d, n2, k, k);
    }
    HIPCHK(c, hipGetLastError());
    return VDET_OK;
}

// Shared tail of nms / vid_nms / track_det_nms on grouped, uploaded data (graph already built):
//   sort -> walk -> survivors of all groups as composites -> global descending sort -> indices.
int nms_grouped_tail(vdet_ctx *c, NmsPlan &pl, const float *d_scores, const uint32_t *d_keys,
                     const uint8_t *d_excl, int64_t *h_keep, int64_t *n_keep)
{
    const int P = (int)pl.groups.size();
    HIPCHK(c, c->keepidx.reserve((size_t)pl.ntot * 4));
    HIPCHK(c, c->keepcnt.reserve((size_t)P * 4));
    SortWalkArgs a{};
    a.mode = 2; a.P = P;
    a.scores = d_scores; a.keys = d_keys; a.excl = d_excl;
    a.keep_idx = c->keepidx.as<int32_t>();
    a.keep_cnt = c->keepcnt.as<int32_t>();
    a.cap = 0;
    int rc = launch_sort_walk(c, a, pl.nmax, pl.ntot);
    if (rc) return rc;
    const uint32_t n2 = pow2ceil((uint32_t)std::max<int64_t>(pl.ntot, 1));
    HIPCHK(c, c->comp.reserve((size_t)n2 * 8));
    HIPCHK(c, hipMemsetAsync(c->comp.p, 0, (size_t)n2 * 8, c->stream));
    hipLaunchKernelGGL(gather_comp_kernel, dim3(P), dim3(256), 0, c->stream, c->groups.as<GroupDesc>(), P,
                       c->keepidx.as<int32_t>(), c->keepcnt.as<int32_t>(), d_scores, d_keys,
                       c->origidx.as<uint32_t>(), c->comp.as<unsigned long long>(), &c->d_cnt->glob_cnt);
    HIPCHK(c, hipGetLastError());
    Counters h;
    HIPCHK(c, hipMemcpyAsync(&h, c->d_cnt, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, host_sync(c));
    rc = translate_status(c, h.status);
    if (rc) return rc;
    const uint32_t nk = h.glob_cnt;
    rc = sort_comp_desc(c, nk);
    if (rc) return rc;
    if (nk) {
        HIPCHK(c, c->out64.reserve((size_t)nk * 8));
        hipLaunchKernelGGL(comp_to_index_kernel, dim3((nk + 255) / 256), dim3(256), 0, c->stream,
                           c->comp.as<unsigned long long>(), nk, c->out64.as<int64_t>());
        HIPCHK(c, hipMemcpyAsync(h_keep, c->out64.p, (size_t)nk * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, host_sync(c));
    }
    *n_keep = nk;
    return VDET_OK;
}

// Group rows by frame value with float32 equality semantics (utils/nms.pyx:111: f_idx[i] != f_idx[j]):
// -0.0 == +0.0; a NaN frame equals nothing, not even itself (singleton groups).
// perm = original indices in grouped order.
int group_by_frame(vdet_ctx *c, const float *frames, int64_t n, int64_t ld, std::vector<int64_t> &perm,
                   std::vector<GroupDesc> &groups)
{
    perm.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) perm[(size_t)i] = i;
    auto key = [&](int64_t i) { return frames[i * ld] + 0.0f; };
    std::stable_sort(perm.begin(), perm.end(), [&](int64_t a, int64_t b) {
        const float fa = key(a), fb = key(b);
        const bool na = fa != fa, nb = fb != fb;
        if (na || nb) return !na && nb;   // NaNs last
        return fa < fb;
    });
    groups.clear();
    int64_t s = 0;
    while (s < n) {
        const float f = key(perm[(size_t)s]);
        int64_t e = s + 1;
        if (f == f)
            while (e < n && key(perm[(size_t)e]) == f) ++e;
        if (e - s > 32767)
            return fail(c, VDET_EINVAL, "%lld detections on one frame; the limit is 32767", (long long)(e - s));
        groups.push_back({(int32_t)s, (int32_t)(e - s), 0});
        s = e;
    }
    return VDET_OK;
}

// ---------------------------------------------------------------------------------------------
// The drop-in calls on <= kFusedMax rows: ONE launch (fused_kernels.hpp).  The rows are packed into host-mapped memory the
// kernel reads directly and the kept list comes back the same way: a call is one launch and one host wait -- no staging
// copies, no scratch shared with the volume entry points (the context's cache stays valid).
// ---------------------------------------------------------------------------------------------
constexpr size_t kFusedInBytes = (size_t)kFusedMax * 6 * 4 + (size_t)kFusedMax * 4 + (size_t)kFusedMaxTracks * 5 * 4;
constexpr size_t kFusedOutBytes = (size_t)(2 + kFusedMax) * 4;

// Wait for a single-launch call by POLLING its "done" words in host-mapped memory (the kernels publish the kept count last,
// release / system scope) instead of hipStreamSynchronize: at T-CNN's call sizes the kernel runs ~15 us and the runtime's
// wake-up was a third of the call (measured through the python module: nms of 100 rows 0.050 -> see INTEGRATION.md).  The done
// words are set to -1 before the launch; hipStreamQuery pushes the launch out; after 2 ms of polling (a long kernel, a busy
// device) the wait falls back to the stream synchronisation, which is also what reports a failed launch.
hipError_t fused_wait(vdet_ctx *c, volatile int32_t *hdr, int64_t K)
{
    ++c->n_host_syncs;
    (void)hipStreamQuery(c->stream);
    const auto t0 = std::chrono::steady_clock::now();
    for (int64_t k = 0; k < K; ++k) {
        unsigned spins = 0;
        while (hdr[2 * k + 1] == -1) {
            __builtin_ia32_pause();
            if ((++spins & 255u) == 0u &&
                std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2))
                return hipStreamSynchronize(c->stream);
        }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    return hipSuccess;
}

int fused_call(vdet_ctx *c, const float *h_rows, int64_t n, int64_t ld, int ncols, double thresh, const int64_t *h_order,
               const float *h_tracks, int64_t t, int64_t ldt, int64_t *h_keep, int64_t *n_keep)
{
    if (!c->fused_in) {
        void *pi = nullptr, *po = nullptr;
        if (hipHostMalloc(&pi, kFusedInBytes, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
            hipHostMalloc(&po, kFusedOutBytes, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) {
            if (pi) (void)hipHostFree(pi);
            return fail(c, VDET_ENOMEM, "host-mapped staging memory for the single-launch calls");
        }
        for (const void *fn : {reinterpret_cast<const void *>(fused_nms_kernel<256>), reinterpret_cast<const void *>(fused_nms_kernel<1024>)}) {
            hipFuncAttributes fa;       // (the dynamic limit is what the kernel's static LDS leaves of the CU's 160 KiB)
            hipError_t e = hipFuncGetAttributes(&fa, fn);
            if (e == hipSuccess)
                e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(c->max_lds - (((size_t)fa.sharedSizeBytes + 15) & ~(size_t)15)));
            if (e != hipSuccess) {
                (void)hipHostFree(pi); (void)hipHostFree(po);
                return fail(c, VDET_EHIP, "hipFuncSetAttribute(fused_nms_kernel) failed: %s", hipGetErrorString(e));
            }
        }
        void *di = nullptr, *dq = nullptr;
        if (hipHostGetDevicePointer(&di, pi, 0) != hipSuccess || hipHostGetDevicePointer(&dq, po, 0) != hipSuccess) {
            (void)hipHostFree(pi); (void)hipHostFree(po);
            return fail(c, VDET_EHIP, "hipHostGetDevicePointer failed for the single-launch staging memory");
        }
        c->fused_in = pi; c->fused_out = po; c->fused_in_dev = di; c->fused_out_dev = dq;
    }
    float *rows = static_cast<float *>(c->fused_in);
    int32_t *rank = reinterpret_cast<int32_t *>(rows + (size_t)kFusedMax * 6);
    float *trk = reinterpret_cast<float *>(rank + kFusedMax);
    volatile int32_t *out = static_cast<volatile int32_t *>(c->fused_out);
    if (ld == ncols) memcpy(rows, h_rows, (size_t)n * ncols * 4);
    else for (int64_t i = 0; i < n; ++i) memcpy(rows + i * ncols, h_rows + i * ld, (size_t)ncols * 4);
    if (h_order) {   // caller-supplied order: priority = position (earlier = higher)
        for (int64_t i = 0; i < n; ++i) rank[i] = 0;
        for (int64_t pos = 0; pos < n; ++pos) {
            const int64_t i = h_order[pos];
            if (i < 0 || i >= n || rank[i]) return fail(c, VDET_EINVAL, "order is not a permutation of 0..n-1");
            rank[i] = (int32_t)(n - pos);
        }
    }
    for (int64_t j = 0; j < t; ++j) memcpy(trk + j * 5, h_tracks + j * ldt, 20);
    FusedParams fp{};
    fp.rows = static_cast<const float *>(c->fused_in_dev);
    fp.rank = h_order ? reinterpret_cast<const int32_t *>(fp.rows + (size_t)kFusedMax * 6) : nullptr;
    fp.tracks = h_tracks ? reinterpret_cast<const float *>(reinterpret_cast<const int32_t *>(fp.rows + (size_t)kFusedMax * 6) + kFusedMax) : nullptr;
    fp.n = (int)n; fp.ncols = ncols; fp.t = (int)t;
    fp.t32 = thresh_to_f32(thresh);
    fp.hdr = static_cast<int32_t *>(c->fused_out_dev);
    fp.kept = fp.hdr + 2;
    int n2 = 64;
    while (n2 < n) n2 <<= 1;
    const size_t lds = fused_lds_bytes((int)n, n2);
    out[1] = -1;                      // the "done" word: the kernel stores the kept count there last
    {
        StageTimer tm(c, ST_WALK);
        if (n <= 128) hipLaunchKernelGGL(fused_nms_kernel<256>, dim3(1), dim3(256), lds, c->stream, fp);
        else hipLaunchKernelGGL(fused_nms_kernel<1024>, dim3(1), dim3(1024), lds, c->stream, fp);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, fused_wait(c, out, 1));
    if (out[0] & kStDivZero) return fail(c, VDET_EDIVZERO, "float division (zero union)");
    const int64_t nk = out[1];
    if (nk < 0 || nk > n) return fail(c, VDET_EHIP, "internal: single-launch NMS returned %lld of %lld rows", (long long)nk, (long long)n);
    for (int64_t k = 0; k < nk; ++k) h_keep[k] = out[2 + k];
    *n_keep = nk;
    return VDET_OK;
}

// K independent track_det_nms problems (vdet/track.py:236-250: one per tracked box, each on its own frame's still-kept
// detections) in ONE launch of K workgroups and ONE host wait.  Host-mapped staging, grown on demand:
//   in : rows [M,6] f32 | tracks [T,5] f32 | off [K+1] i32 | toff [K+1] i32         out: hdr [K,2] i32 | kept [M] i32
int fused_batch_call(vdet_ctx *c, const float *h_tracks, const int64_t *h_toff, int64_t ldt, const float *h_dets, const int64_t *h_off,
                     int64_t K, int64_t ldd, double thresh, int64_t *h_keep, int64_t *h_nkeep, int64_t max_m)
{
    const int64_t M = h_off[K], T = h_toff ? h_toff[K] : K;
    const size_t in_bytes = (((size_t)M * 24 + (size_t)T * 20 + 15) & ~(size_t)15) + 2 * (size_t)(K + 1) * 4;
    const size_t out_bytes = (size_t)K * 8 + (size_t)M * 4;
    if (in_bytes > c->fbatch_in_cap || out_bytes > c->fbatch_out_cap) {
        if (c->fbatch_in) (void)hipHostFree(c->fbatch_in);
        if (c->fbatch_out) (void)hipHostFree(c->fbatch_out);
        c->fbatch_in = c->fbatch_out = c->fbatch_in_dev = c->fbatch_out_dev = nullptr;
        c->fbatch_in_cap = c->fbatch_out_cap = 0;
        const size_t ci = std::max<size_t>(in_bytes + in_bytes / 2, (size_t)1 << 20), co = std::max<size_t>(out_bytes + out_bytes / 2, (size_t)1 << 18);
        void *pi = nullptr, *po = nullptr, *di = nullptr, *dq = nullptr;
        if (hipHostMalloc(&pi, ci, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
            hipHostMalloc(&po, co, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) {
            if (pi) (void)hipHostFree(pi);
            return fail(c, VDET_ENOMEM, "host-mapped staging memory for vdet_track_det_nms_batch");
        }
        if (hipHostGetDevicePointer(&di, pi, 0) != hipSuccess || hipHostGetDevicePointer(&dq, po, 0) != hipSuccess) {
            (void)hipHostFree(pi); (void)hipHostFree(po);
            return fail(c, VDET_EHIP, "hipHostGetDevicePointer failed for the batch staging memory");
        }
        c->fbatch_in = pi; c->fbatch_out = po; c->fbatch_in_dev = di; c->fbatch_out_dev = dq;
        c->fbatch_in_cap = ci; c->fbatch_out_cap = co;
    }
    if (!c->fbatch_attr) {
        for (const void *fn : {reinterpret_cast<const void *>(fused_nms_batch_kernel<256>), reinterpret_cast<const void *>(fused_nms_batch_kernel<1024>)}) {
            hipFuncAttributes fa;
            hipError_t e = hipFuncGetAttributes(&fa, fn);
            if (e == hipSuccess)
                e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(c->max_lds - (((size_t)fa.sharedSizeBytes + 15) & ~(size_t)15)));
            if (e != hipSuccess) return fail(c, VDET_EHIP, "hipFuncSetAttribute(fused_nms_batch_kernel) failed: %s", hipGetErrorString(e));
        }
        c->fbatch_attr = true;
    }
    float *rows = static_cast<float *>(c->fbatch_in);
    float *trk = rows + (size_t)M * 6;
    const size_t tab = ((size_t)M * 24 + (size_t)T * 20 + 15) & ~(size_t)15;
    int32_t *off = reinterpret_cast<int32_t *>(static_cast<unsigned char *>(c->fbatch_in) + tab);
    int32_t *toff = off + (K + 1);
    if (ldd == 6) memcpy(rows, h_dets, (size_t)M * 24);
    else for (int64_t i = 0; i < M; ++i) memcpy(rows + i * 6, h_dets + i * ldd, 24);
    for (int64_t j = 0; j < T; ++j) memcpy(trk + j * 5, h_tracks + j * ldt, 20);
    for (int64_t k = 0; k <= K; ++k) { off[k] = (int32_t)h_off[k]; toff[k] = (int32_t)(h_toff ? h_toff[k] : k); }
    volatile int32_t *hdr = static_cast<volatile int32_t *>(c->fbatch_out);
    volatile int32_t *kept = hdr + 2 * K;
    FusedBatchParams bp{};
    const unsigned char *din = static_cast<const unsigned char *>(c->fbatch_in_dev);
    bp.rows = reinterpret_cast<const float *>(din);
    bp.tracks = bp.rows + (size_t)M * 6;
    bp.off = reinterpret_cast<const int32_t *>(din + tab);
    bp.toff = bp.off + (K + 1);
    bp.t32 = thresh_to_f32(thresh);
    bp.hdr = static_cast<int32_t *>(c->fbatch_out_dev);
    bp.kept = bp.hdr + 2 * K;
    int n2 = 64;
    while (n2 < max_m) n2 <<= 1;
    const size_t lds = fused_lds_bytes((int)std::max<int64_t>(max_m, 1), n2);
    for (int64_t k = 0; k < K; ++k) hdr[2 * k + 1] = -1;      // the problems' "done" words
    {
        StageTimer tm(c, ST_WALK);
        if (max_m <= 128) hipLaunchKernelGGL(fused_nms_batch_kernel<256>, dim3((unsigned)K), dim3(256), lds, c->stream, bp);
        else hipLaunchKernelGGL(fused_nms_batch_kernel<1024>, dim3((unsigned)K), dim3(1024), lds, c->stream, bp);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, fused_wait(c, hdr, K));
    bool divz = false;
    for (int64_t k = 0; k < K; ++k) {
        const int64_t m = h_off[k + 1] - h_off[k], nk = hdr[2 * k + 1];
        if (hdr[2 * k] & kStDivZero) divz = true;
        if (nk < 0 || nk > m) return fail(c, VDET_EHIP, "internal: batched single-launch NMS returned %lld of %lld rows", (long long)nk, (long long)m);
        h_nkeep[k] = nk;
        for (int64_t q = 0; q < nk; ++q) h_keep[h_off[k] + q] = kept[h_off[k] + q];
    }
    if (divz) return fail(c, VDET_EDIVZERO, "float division (zero union)");
    return VDET_OK;
}

}  // namespace

// =============================================================================================
// C-ABI
// =============================================================================================
extern "C" {

const char *vdet_version(void) { return "vdet_hip 0.1 gfx950"; }

int vdet_create(vdet_ctx **out, int device)
{
    if (!out) return VDET_EINVAL;
    *out = nullptr;
    vdet_ctx *c = new (std::nothrow) vdet_ctx;
    if (!c) return VDET_ENOMEM;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        delete c;
        return VDET_EHIP;   // fail loudly: there is NO CPU fallback in this library
    }
    if (device < 0) {
        if (hipGetDevice(&device) != hipSuccess) { delete c; return VDET_EHIP; }
    }
    if (device >= ndev || hipSetDevice(device) != hipSuccess) { delete c; return VDET_EINVAL; }
    c->device = device;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) {
        c->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        // gfx950: one workgroup may own the CU's whole 160 KiB LDS (opt-in via hipFuncSetAttribute)
        if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) c->max_lds = 64 * 1024;
    }
    if (const char *e = getenv("VDET_FORCE_GENERAL")) c->force_general = atoi(e) != 0;
    if (const char *e = getenv("VDET_BITS_BUDGET_MB")) {
        const long mb = atol(e);
        if (mb > 0) c->bits_budget = (size_t)mb << 20;
    }
    if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess ||
        hipMalloc((void **)&c->d_cnt, sizeof(Counters)) != hipSuccess) {
        delete c;
        return VDET_EHIP;
    }
    c->stream = c->own_stream;
    (void)hipMemsetAsync(c->d_cnt, 0, sizeof(Counters), c->stream);
    if (const char *e = getenv("VDET_NO_INDEX")) c->no_index = atoi(e) != 0;
    if (const char *e = getenv("VDET_NO_LAZY")) c->no_lazy = atoi(e) != 0;
    if (const char *e = getenv("VDET_NO_FUSED")) c->no_fused = atoi(e) != 0;
    if (const char *e = getenv("VDET_ADJ_ROWS")) c->adj_rows = atoi(e) != 0;
    if (const char *e = getenv("VDET_DIRECT_LISTS")) c->direct_lists = atoi(e) != 0;
    if (const char *e = getenv("VDET_DIRECT_CAP")) { const int v = atoi(e); if (v >= 8 && v <= 32760) c->direct_cap = (uint32_t)(v & ~7); }
    if (const char *e = getenv("VDET_BINSORT")) c->binsort = atoi(e) != 0;
    if (const char *e = getenv("VDET_BINSORT_INHERIT")) c->binsort_inherit = atoi(e) != 0;
    if (const char *e = getenv("VDET_WALK_WIDE")) { if (atoi(e) == 0) c->walk_wide_nsw = 0; }
    if (const char *e = getenv("VDET_WALK_WIDE_NSW")) { const int v = atoi(e); if (v >= 1 && v <= 63 && c->walk_wide_nsw > 0) c->walk_wide_nsw = v; }
    if (const char *e = getenv("VDET_BINSORT_GRID")) { const int v = atoi(e); if (v >= 1) c->binsort_grid = v; }
    if (const char *e = getenv("VDET_SMALL_LISTS")) c->small_lists = atoi(e) != 0;
    if (const char *e = getenv("VDET_TCN_TILED")) c->tcn_tiled = atoi(e) != 0;
    if (const char *e = getenv("VDET_TCN_GLOBAL")) c->tcn_global = atoi(e) != 0;
    if (const char *e = getenv("VDET_CTX_RECORDS")) c->ctxs_records = atoi(e) != 0;
    if (const char *e = getenv("VDET_SEQNMS_LDS")) c->sq_lds = atoi(e) != 0;
    if (const char *e = getenv("VDET_VPASS_FORM")) { const int v = atoi(e); if (v >= VDET_VPASS_AUTO && v <= VDET_VPASS_ONE_PER_CU) c->vpass_form = v; }
    if (const char *e = getenv("VDET_VPASS_FCHUNK")) { const int v = atoi(e); if (v >= 1) c->vpass_fchunk = v; }
    {   // probe: do returning LDS atomics resolve same-address lanes in ascending lane order?
        const int npat = 4096;
        std::vector<uint8_t> pats((size_t)npat * 64);
        uint32_t rs = 12345u;
        auto rnd = [&]() { rs = rs * 1664525u + 1013904223u; return rs >> 8; };
        for (int t = 0; t < npat; ++t) {
            const int kind = t % 8;
            const int nd = kind == 0 ? 1 : kind == 1 ? 2 : kind == 2 ? 3 : kind == 3 ? 8 : kind == 4 ? 32 : kind == 5 ? 64 : kind == 6 ? 200 : 254;
            for (int l = 0; l < 64; ++l) {
                uint8_t d = (uint8_t)(rnd() % nd);
                if (kind == 7 && (rnd() & 3) == 0) d = 255;          // inactive lanes
                if (t % 16 == 9) d = (uint8_t)((l * (1 + t % 7)) % nd); // structured strides
                pats[(size_t)t * 64 + l] = d;
            }
        }
        bool ok = false;
        DevBuf pb;
        if (pb.reserve(pats.size()) == hipSuccess &&
            hipMemcpyAsync(pb.p, pats.data(), pats.size(), hipMemcpyHostToDevice, c->stream) == hipSuccess) {
            hipLaunchKernelGGL(lds_atomic_order_probe, dim3(256), dim3(64), 0, c->stream, pb.as<uint8_t>(), npat,
                               &c->d_cnt->status);
            Counters h;
            if (hipMemcpyAsync(&h, c->d_cnt, sizeof h, hipMemcpyDeviceToHost, c->stream) == hipSuccess &&
                host_sync(c) == hipSuccess)
                ok = (h.status == 0);
        }
        pb.release();
        (void)hipMemsetAsync(c->d_cnt, 0, sizeof(Counters), c->stream);
        c->atomic_rank = ok;
        if (const char *e = getenv("VDET_ATOMIC_RANK")) c->atomic_rank = c->atomic_rank && atoi(e) != 0;
    }
    {   // does wave_transpose64 (K1s's transposed emission) behave as derived on this device?
        const int n = 64;
        std::vector<uint64_t> hin((size_t)n * 64), hout((size_t)n * 64);
        uint64_t x = 0x9E3779B97F4A7C15ull;
        for (size_t i = 0; i < hin.size(); ++i) {
            x ^= x << 13; x ^= x >> 7; x ^= x << 17;
            hin[i] = (i / 64) == 0 ? (1ull << (i % 64)) : ((i / 64) == 1 ? (uint64_t)(i % 64 == 5 ? ~0ull : 0ull) : x);
        }
        bool ok = false;
        DevBuf bi, bo;
        if (bi.reserve(hin.size() * 8) == hipSuccess && bo.reserve(hin.size() * 8) == hipSuccess &&
            hipMemcpyAsync(bi.p, hin.data(), hin.size() * 8, hipMemcpyHostToDevice, c->stream) == hipSuccess) {
            hipLaunchKernelGGL(wave_transpose_probe, dim3(16), dim3(64), 0, c->stream, bi.as<uint64_t>(), bo.as<uint64_t>(), n);
            if (hipMemcpyAsync(hout.data(), bo.p, hout.size() * 8, hipMemcpyDeviceToHost, c->stream) == hipSuccess &&
                host_sync(c) == hipSuccess) {
                ok = true;
                for (int t = 0; t < n && ok; ++t)
                    for (int r = 0; r < 64 && ok; ++r)
                        for (int k = 0; k < 64; ++k)
                            if (((hin[(size_t)t * 64 + r] >> k) & 1ull) != ((hout[(size_t)t * 64 + k] >> r) & 1ull)) { ok = false; break; }
            }
        }
        bi.release(); bo.release();
        c->wave_transpose = ok;
        if (const char *e = getenv("VDET_WAVE_TRANSPOSE")) c->wave_transpose = c->wave_transpose && atoi(e) != 0;
    }
    *out = c;
    return VDET_OK;
}

int vdet_destroy(vdet_ctx *c)
{
    if (!c) return VDET_OK;
    (void)hipSetDevice(c->device);
    (void)host_sync(c);
    DevBuf *bufs[] = {&c->boxes, &c->scores, &c->keys, &c->excl, &c->frames, &c->groups, &c->tiles, &c->bits,
                      &c->rowz, &c->rowmeta, &c->groupz, &c->adj, &c->comp, &c->origidx, &c->out64,
                      &c->trk_frames, &c->trk_boxes, &c->b1, &c->b2, &c->iou_out, &c->order, &c->ncand, &c->keepidx,
                      &c->keepcnt, &c->gflags, &c->pairs, &c->tkeys, &c->tstate, &c->visited, &c->heads, &c->xkeys, &c->xord, &c->xncand, &c->linkmemo, &c->linkstats, &c->linkwarm, &c->linkorder, &c->linkchains, &c->linknodes, &c->tracknode, &c->rtodo,
                      &c->xbox, &c->xbox16, &c->xord16, &c->xcum, &c->xinfo, &c->wmeta, &c->wmeta16, &c->reachtab, &c->rowperm, &c->qreach, &c->ditems, &c->striptot, &c->stripoff, &c->sortctl, &c->walkstats, &c->segtab.dev, &c->vidtab.dev, &c->nover, &c->ordncand, &c->ev_tab, &c->ev_dtp, &c->ev_dsc,
                      &c->ev_dslot, &c->ev_bcnt, &c->ev_boff, &c->ev_key[0], &c->ev_key[1], &c->ev_val[0], &c->ev_val[1], &c->ev_hist,
                      &c->tcn_x, &c->tcn_frames, &c->tcn_base, &c->tcn_len, &c->tcn_scratch, &c->tcn_h0, &c->tcn_params.dev, &c->tcn_foff.dev, &c->tcn_segs.dev, &c->tcn_ovtab.dev, &c->interp_tab.dev,
                      &c->anchor_tab.dev, &c->topa_hist, &c->topa_state, &c->topa_cnt, &c->topa_nrec, &c->topa_rec, &c->svm_wt, &c->svm_wavebad,
                      &c->ctxs_tab.dev, &c->ctxs_hist, &c->ctxs_state, &c->ctxs_rec, &c->sq_link, &c->sq_live, &c->sq_done, &c->sq_ptr, &c->tube_scratch,
                      &c->rpn_keys, &c->rpn_boxes, &c->rpn_cbox, &c->rpn_cscore, &c->rpn_cindex, &c->rpn_order, &c->rpn_ccnt, &c->rpn_keep, &c->rpn_keepcnt};
    for (DevBuf *b : bufs) b->release();
    for (DevBuf &b : c->tmp) b.release();
    for (auto &e : c->ev_pool) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    if (c->d_cnt) (void)hipFree(c->d_cnt);
    if (c->fused_in) (void)hipHostFree(c->fused_in);
    if (c->fused_out) (void)hipHostFree(c->fused_out);
    if (c->fbatch_in) (void)hipHostFree(c->fbatch_in);
    if (c->fbatch_out) (void)hipHostFree(c->fbatch_out);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
    return VDET_OK;
}

int vdet_set_stream(vdet_ctx *c, void *s)
{
    if (!c) return VDET_EINVAL;
    c->stream = (hipStream_t)s;        // verbatim: NULL is HIP's null stream (torch's default stream)
    return VDET_OK;
}

int vdet_reset_stream(vdet_ctx *c)
{
    if (!c) return VDET_EINVAL;
    c->stream = c->own_stream;
    return VDET_OK;
}

const char *vdet_last_error(vdet_ctx *c) { return c ? c->err.c_str() : "null context"; }

int vdet_set_cache(vdet_ctx *c, int enable)
{
    if (!c) return VDET_EINVAL;
    c->cache_enabled = enable != 0;
    c->graph_valid = c->lists_valid = c->index_valid = c->keys_valid = c->nodes_valid = false;
    return VDET_OK;
}

int vdet_invalidate(vdet_ctx *c)
{
    if (!c) return VDET_EINVAL;
    c->graph_valid = c->lists_valid = c->index_valid = c->keys_valid = c->nodes_valid = false;
    return VDET_OK;
}

int vdet_query(vdet_ctx *c, int what)
{
    if (!c) return VDET_EINVAL;
    if (what == 0) return c->atomic_rank ? 1 : 0;
    if (what == 1) return c->n_cu;
    if (what == 2) return c->all_regular ? 1 : 0;
    if (what == 3) return c->wave_transpose ? 1 : 0;
    if (what == 15) return c->direct_ntot > 0 ? 1 : 0;    // the last graph build took the direct lists (graph_lists_kernel)
    if (what == 8) return (int)std::min<long long>(c->n_host_syncs, 0x7FFFFFFF);
    if (what == 10) return (int)std::min<long long>(c->tcn_params.uploads, 0x7FFFFFFF);   // TCN parameter uploads so far
    if (what == 11) return (int)std::min<long long>(c->anchor_tab.uploads, 0x7FFFFFFF);   // per-video tables of the anchor route's batch forms staged so far
    if (what == 12) return c->vpass_last_items;   // 4: the current fused kernel, 2: the lean one, 0: the separate temporal kernels; + 100: one block per unit
    if (what == 13) {  // full reads of the volume the last vdet_context_classes needed (-1: no call yet)
        if (c->ctxs_last_videos <= 0 || !c->ctxs_state.p) return -1;
        std::vector<CtxState> h((size_t)c->ctxs_last_videos);
        if (hipMemcpyAsync(h.data(), c->ctxs_state.p, h.size() * sizeof(CtxState), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            host_sync(c) != hipSuccess) return VDET_EHIP;
        int reads = 0;
        for (const CtxState &st : h) reads = std::max(reads, st.empty ? 0 : 2 + (int)st.path);
        return reads;
    }
    if (what == 14) return c->sq_last_path;   // the last vdet_seq_nms[_batch]: 1 predecessor table in LDS, 2 in global scratch (-1: no call yet)
    if (what == 9 || what == 16 || what == 17) {   // the last volume sort's counting kernel (-1: it did not run): problems handed to
        // the LSD kernel (9), sorted with an inherited key -> bin map (16), sorted again with their own map (17)
        if (!c->last_sort_binned || !c->sortctl.p) return -1;
        BinSortCtl h{};
        if (hipMemcpyAsync(&h, c->sortctl.p, sizeof h, hipMemcpyDeviceToHost, c->stream) != hipSuccess || host_sync(c) != hipSuccess) return VDET_EHIP;
        return what == 9 ? h.nfail : what == 16 ? h.ninherit : h.nredo;
    }
    if (what == 18 || what == 19) {   // the last volume walk's wide filter (-1: it could not run): lists that entered it (18), wide
        // passes that wanted more candidates than the staging holds and were queued slice by slice (19)
        if (!c->last_walk_wide || !c->walkstats.p) return -1;
        uint32_t h[2 * kWideStatSlots];
        if (hipMemcpyAsync(h, c->walkstats.p, sizeof h, hipMemcpyDeviceToHost, c->stream) != hipSuccess || host_sync(c) != hipSuccess) return VDET_EHIP;
        unsigned long long n = 0;
        for (int i = 0; i < kWideStatSlots; ++i) n += h[(what - 18) * kWideStatSlots + i];
        return (int)std::min<unsigned long long>(n, 0x7FFFFFFFull);
    }
    if (what >= 4 && what <= 7) {     // link steps of the last tracking call served by the memo (4) / scanned (5); 6 / 7: the warm-up's
        unsigned int h[4] = {0, 0, 0, 0};
        if (!c->linkstats.p) return 0;
        if (hipMemcpyAsync(h, c->linkstats.p, 16, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            host_sync(c) != hipSuccess) return VDET_EHIP;
        return (int)std::min<unsigned int>(h[what - 4], 0x7FFFFFFFu);
    }
    return VDET_EINVAL;
}

int vdet_set_timing(vdet_ctx *c, int enable)
{
    if (!c) return VDET_EINVAL;
    c->timing = enable != 0;
    c->timing_accumulate = enable == 2;
    c->ev_used = 0;
    return VDET_OK;
}

int vdet_last_timing_ms(vdet_ctx *c, float *out16)
{
    float *out8 = out16;
    if (!c || !out8) return VDET_EINVAL;
    HIPCHK(c, host_sync(c));
    for (int i = 0; i < ST_COUNT; ++i) { c->last_ms[i] = 0; c->last_launches[i] = 0; }
    for (size_t i = 0; i < c->ev_used; ++i) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, c->ev_pool[i].first, c->ev_pool[i].second) == hipSuccess) {
            c->last_ms[c->ev_stage[i]] += ms;
            c->last_launches[c->ev_stage[i]] += 1;
        }
    }
    for (int i = 0; i < ST_COUNT; ++i) out8[i] = c->last_ms[i];
    c->ev_used = 0;
    return VDET_OK;
}

int vdet_last_launches(vdet_ctx *c, int *out16)
{
    if (!c || !out16) return VDET_EINVAL;
    for (int i = 0; i < ST_COUNT; ++i) out16[i] = c->last_launches[i];
    return VDET_OK;
}

int vdet_sync(vdet_ctx *c)
{
    if (!c) return VDET_EINVAL;
    Counters h;
    HIPCHK(c, hipMemcpyAsync(&h, c->d_cnt, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, host_sync(c));
    HIPCHK(c, hipMemsetAsync(&c->d_cnt->status, 0, kPerBuildOff, c->stream));     // status, eindex, pool_max
    h.pool_used = std::max(h.pool_used, h.pool_max);
    const int l = c->latched;
    c->latched = 0;
    if ((h.status & kStPoolAsync) || l == VDET_EAGAIN) {
        // an asynchronous graph build (vdet_set_async) ran out of adjacency pool: everything enqueued
        // since is invalid.  The pool is enlarged here, so running the same calls again succeeds.
        // (handled before a latched error of the same window is reported: the truncated graph must not be reused)
        c->graph_valid = c->lists_valid = c->nodes_valid = false;
        if (h.status & kStDirect) {      // a direct slot overflowed: the bit-matrix path from now on, its pool sized from the cursors
            c->direct_lists = false;
            unsigned long long need = 0ull;
            if (c->direct_ntot > 0 && c->striptot.reserve(8) == hipSuccess &&
                hipMemsetAsync(c->striptot.p, 0, 8, c->stream) == hipSuccess) {
                hipLaunchKernelGGL(deg_sum_kernel, dim3(1024), dim3(256), 0, c->stream, c->rowz.as<uint32_t>(), c->direct_ntot,
                                   c->striptot.as<unsigned long long>());
                if (hipMemcpyAsync(&need, c->striptot.p, 8, hipMemcpyDeviceToHost, c->stream) != hipSuccess || host_sync(c) != hipSuccess) need = 0ull;
            }
            const unsigned long long dyn = h.pool_used > c->direct_fixed ? h.pool_used - c->direct_fixed : 0ull;
            h.pool_used = need + dyn + 4096;
            c->pool_hint = 0;            // (the hint of the direct builds counted the fixed slots)
        }
        c->pool_hint = std::max(c->pool_hint, h.pool_used);
        if (h.pool_used <= 0xFFFFFFFFull) (void)c->adj.reserve((size_t)(h.pool_used + h.pool_used / 2) * 2 + 4096);
        if (l && l != VDET_EAGAIN) return l;
        return fail(c, VDET_EAGAIN, "adjacency pool overflow in an asynchronous graph build (%llu entries needed): the "
                                    "results since the last vdet_sync are invalid; the pool has been enlarged, run the calls again",
                    (unsigned long long)h.pool_used);
    }
    if (l) return l;
    c->pool_hint = std::max(c->pool_hint, h.pool_used);
    if (h.eindex) return fail(c, VDET_EINDEX, "list index out of range");
    return translate_status(c, h.status);
}

int vdet_set_async(vdet_ctx *c, int enable)
{
    if (!c) return VDET_EINVAL;
    c->async_enabled = enable != 0;
    return VDET_OK;
}

int vdet_set_vpass(vdet_ctx *c, int form, int fchunk)
{
    if (!c) return VDET_EINVAL;
    if (form < VDET_VPASS_AUTO || form > VDET_VPASS_ONE_PER_CU || fchunk < 0) return fail(c, VDET_EINVAL, "bad volume pass form");
    c->vpass_form = form;
    c->vpass_fchunk = fchunk;
    return VDET_OK;
}

// ---------------------------------------------------------------------------------------------
int vdet_nms_f32(vdet_ctx *c, const float *h_dets, int64_t n, int64_t ld, int ncols, double thresh,
                 const int64_t *h_order, int64_t *h_keep, int64_t *n_keep)
{
    if (!c || !n_keep) return VDET_EINVAL;
    *n_keep = 0;
    if (n < 0 || (ncols != 5 && ncols != 6) || (n > 0 && (!h_dets || !h_keep || ld < ncols)))
        return fail(c, VDET_EINVAL, "dets must be float32 [n,%d]", ncols);
    if (n == 0) return VDET_OK;
    if (n > 0x7FFFFFFF) return fail(c, VDET_EINVAL, "too many detections");
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    if (n <= kFusedMax && !c->no_fused)      // the T-CNN call sizes: one launch (fused_kernels.hpp)
        return fused_call(c, h_dets, n, ld, ncols, thresh, h_order, nullptr, 0, 0, h_keep, n_keep);
    const int o = ncols == 6 ? 1 : 0;

    NmsPlan pl;
    std::vector<int64_t> perm;
    if (o) {
        int rc = group_by_frame(c, h_dets, n, ld, perm, pl.groups);
        if (rc) return rc;
    } else {
        if (n > 32767) return fail(c, VDET_EINVAL, "%lld boxes in one image; the limit is 32767", (long long)n);
        perm.resize((size_t)n);
        for (int64_t i = 0; i < n; ++i) perm[(size_t)i] = i;
        pl.groups.push_back({0, (int32_t)n, 0});
    }
    make_plan(c, pl);

    std::vector<float> hb((size_t)n * 4), hs((size_t)n);
    std::vector<uint32_t> hidx((size_t)n), hkeys;
    for (int64_t r = 0; r < n; ++r) {
        const float *row = h_dets + perm[(size_t)r] * ld + o;
        memcpy(&hb[(size_t)r * 4], row, 16);
        hs[(size_t)r] = row[4];
        hidx[(size_t)r] = (uint32_t)perm[(size_t)r];
    }
    if (h_order) {   // caller-supplied order: priority = position (earlier = higher)
        std::vector<uint32_t> rank((size_t)n, 0);
        for (int64_t pos = 0; pos < n; ++pos) {
            const int64_t i = h_order[pos];
            if (i < 0 || i >= n || rank[(size_t)i]) return fail(c, VDET_EINVAL, "order is not a permutation of 0..n-1");
            rank[(size_t)i] = (uint32_t)(n - pos);
        }
        hkeys.resize((size_t)n);
        for (int64_t r = 0; r < n; ++r) hkeys[(size_t)r] = rank[(size_t)perm[(size_t)r]];
    }
    HIPCHK(c, c->boxes.reserve((size_t)n * 16));
    HIPCHK(c, c->scores.reserve((size_t)n * 4));
    HIPCHK(c, c->origidx.reserve((size_t)n * 4));
    HIPCHK(c, hipMemcpyAsync(c->boxes.p, hb.data(), (size_t)n * 16, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->scores.p, hs.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->origidx.p, hidx.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    const uint32_t *d_keys = nullptr;
    if (h_order) {
        HIPCHK(c, c->keys.reserve((size_t)n * 4));
        HIPCHK(c, hipMemcpyAsync(c->keys.p, hkeys.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
        d_keys = c->keys.as<uint32_t>();
    }
    HIPCHK(c, host_sync(c));
    // the graph / lists / index of an earlier d_* call are overwritten below (shared scratch)
    c->graph_valid = c->lists_valid = c->index_valid = false;
    HostGroupsGuard guard(c);
    int rc = build_graph(c, c->boxes.as<float4>(), pl, thresh_to_f32(thresh), thresh, false);
    if (rc) return rc;
    return nms_grouped_tail(c, pl, c->scores.as<float>(), d_keys, nullptr, h_keep, n_keep);
}

int vdet_track_det_nms_f32(vdet_ctx *c, const float *h_tracks, int64_t t, int64_t ldt, const float *h_dets,
                           int64_t m, int64_t ldd, double thresh, int64_t *h_keep, int64_t *n_keep)
{
    if (!c || !n_keep) return VDET_EINVAL;
    *n_keep = 0;
    if (t < 0 || m < 0 || (t > 0 && (!h_tracks || ldt < 5)) || (m > 0 && (!h_dets || !h_keep || ldd < 6)))
        return fail(c, VDET_EINVAL, "tracks must be float32 [t,5], dets float32 [m,6]");
    if (m == 0) return VDET_OK;
    if (m > 0x7FFFFFFF || t > 0x7FFFFFFF) return fail(c, VDET_EINVAL, "too many rows");
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    if (m <= kFusedMax && t <= kFusedMaxTracks && !c->no_fused)      // the T-CNN call sizes: one launch (fused_kernels.hpp)
        return fused_call(c, h_dets, m, ldd, 6, thresh, nullptr, t > 0 ? h_tracks : nullptr, t, ldt, h_keep, n_keep);
    NmsPlan pl;
    std::vector<int64_t> perm;
    int rc = group_by_frame(c, h_dets, m, ldd, perm, pl.groups);
    if (rc) return rc;
    make_plan(c, pl);
    std::vector<float> hb((size_t)m * 4), hs((size_t)m), hf((size_t)m);
    std::vector<uint32_t> hidx((size_t)m);
    for (int64_t r = 0; r < m; ++r) {
        const float *row = h_dets + perm[(size_t)r] * ldd;
        hf[(size_t)r] = row[0];
        memcpy(&hb[(size_t)r * 4], row + 1, 16);
        hs[(size_t)r] = row[5];
        hidx[(size_t)r] = (uint32_t)perm[(size_t)r];
    }
    std::vector<float> tb((size_t)std::max<int64_t>(t, 1) * 4), tf((size_t)std::max<int64_t>(t, 1));
    for (int64_t j = 0; j < t; ++j) {
        tf[(size_t)j] = h_tracks[j * ldt];
        memcpy(&tb[(size_t)j * 4], h_tracks + j * ldt + 1, 16);
    }
    const float t32 = thresh_to_f32(thresh);
    HIPCHK(c, c->boxes.reserve((size_t)m * 16));
    HIPCHK(c, c->scores.reserve((size_t)m * 4));
    HIPCHK(c, c->frames.reserve((size_t)m * 4));
    HIPCHK(c, c->origidx.reserve((size_t)m * 4));
    HIPCHK(c, c->excl.reserve((size_t)m));
    HIPCHK(c, c->trk_boxes.reserve(tb.size() * 4));
    HIPCHK(c, c->trk_frames.reserve(tf.size() * 4));
    HIPCHK(c, hipMemcpyAsync(c->boxes.p, hb.data(), (size_t)m * 16, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->scores.p, hs.data(), (size_t)m * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->frames.p, hf.data(), (size_t)m * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->origidx.p, hidx.data(), (size_t)m * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->trk_boxes.p, tb.data(), tb.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->trk_frames.p, tf.data(), tf.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, host_sync(c));
    c->graph_valid = c->lists_valid = c->index_valid = false;     // shared scratch is overwritten below
    HostGroupsGuard guard(c);
    // build_graph clears the status word, so round 1 runs after it (inside the same stream order):
    rc = build_graph(c, c->boxes.as<float4>(), pl, t32, thresh, false);
    if (rc) return rc;
    {
        StageTimer tm(c, ST_OTHER);
        hipLaunchKernelGGL(track_round1_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, c->stream,
                           c->frames.as<float>(), c->boxes.as<float4>(), (int)m, c->trk_frames.as<float>(),
                           c->trk_boxes.as<float4>(), (int)t, t32, c->excl.as<uint8_t>(), &c->d_cnt->status);
    }
    HIPCHK(c, hipGetLastError());
    return nms_grouped_tail(c, pl, c->scores.as<float>(), nullptr, c->excl.as<uint8_t>(), h_keep, n_keep);
}


int vdet_track_det_nms_batch(vdet_ctx *c, const float *h_tracks, const int64_t *h_toff, int64_t ldt, const float *h_dets,
                             const int64_t *h_off, int64_t K, int64_t ldd, double thresh, int64_t *h_keep, int64_t *h_nkeep)
{
    if (!c) return VDET_EINVAL;
    if (K < 0 || (K > 0 && (!h_off || !h_nkeep))) return fail(c, VDET_EINVAL, "need K >= 0 problems with offsets and a count per problem");
    if (K == 0) return VDET_OK;
    if (K > 0x3FFFFFFF || h_off[0] != 0 || (h_toff && h_toff[0] != 0)) return fail(c, VDET_EINVAL, "offsets must start at 0");
    int64_t max_m = 0, max_t = 0;
    for (int64_t k = 0; k < K; ++k) {
        const int64_t m = h_off[k + 1] - h_off[k], t = h_toff ? h_toff[k + 1] - h_toff[k] : 1;
        if (m < 0 || t < 0) return fail(c, VDET_EINVAL, "offsets must not decrease");
        max_m = std::max(max_m, m); max_t = std::max(max_t, t);
        h_nkeep[k] = 0;
    }
    const int64_t M = h_off[K], T = h_toff ? h_toff[K] : K;
    if (M > 0x7FFFFFFF || T > 0x7FFFFFFF) return fail(c, VDET_EINVAL, "too many rows");
    if ((T > 0 && (!h_tracks || ldt < 5)) || (M > 0 && (!h_dets || !h_keep || ldd < 6)))
        return fail(c, VDET_EINVAL, "tracks must be float32 [T,5], dets float32 [M,6]");
    if (M == 0) return VDET_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if (max_m <= kFusedMax && max_t <= kFusedMaxTracks && !c->no_fused) {
        timing_reset(c);
        return fused_batch_call(c, h_tracks, h_toff, ldt, h_dets, h_off, K, ldd, thresh, h_keep, h_nkeep, max_m);
    }
    // a problem beyond the single-launch sizes (or VDET_NO_FUSED=1): the problems one by one through the general chain
    for (int64_t k = 0; k < K; ++k) {
        const int64_t t0 = h_toff ? h_toff[k] : k, t = h_toff ? h_toff[k + 1] - h_toff[k] : 1;
        const int rc = vdet_track_det_nms_f32(c, h_tracks ? h_tracks + t0 * ldt : nullptr, t, ldt, h_dets + h_off[k] * ldd, h_off[k + 1] - h_off[k], ldd, thresh,
                                              h_keep + h_off[k], &h_nkeep[k]);
        if (rc) return rc;
    }
    return VDET_OK;
}

int vdet_iou_f64(vdet_ctx *c, const double *h_b1, int64_t n1, const double *h_b2, int64_t n2, double *h_out)
{
    if (!c || n1 < 0 || n2 < 0) return VDET_EINVAL;
    if (n1 == 0 || n2 == 0) return VDET_OK;
    if (!h_b1 || !h_b2 || !h_out) return fail(c, VDET_EINVAL, "null buffer");
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    HIPCHK(c, c->b1.reserve((size_t)n1 * 32));
    HIPCHK(c, c->b2.reserve((size_t)n2 * 32));
    HIPCHK(c, c->iou_out.reserve((size_t)n1 * n2 * 8));
    HIPCHK(c, hipMemcpyAsync(c->b1.p, h_b1, (size_t)n1 * 32, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->b2.p, h_b2, (size_t)n2 * 32, hipMemcpyHostToDevice, c->stream));
    {
        StageTimer tm(c, ST_OTHER);
        hipLaunchKernelGGL(iou_f64_kernel, dim3((unsigned)((n2 + 255) / 256), (unsigned)std::min<int64_t>(n1, 4096)),
                           dim3(256), 0, c->stream, c->b1.as<double>(), n1, c->b2.as<double>(), n2,
                           c->iou_out.as<double>());
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h_out, c->iou_out.p, (size_t)n1 * n2 * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, host_sync(c));
    return VDET_OK;
}

// ---------------------------------------------------------------------------------------------
int vdet_nms_volume(vdet_ctx *c, const float *d_boxes, const float *d_scores, int layout, int64_t F, int64_t B,
                    int64_t C, double thresh, int use_score_thresh, float score_thresh, int32_t *d_keep_idx,
                    int32_t *d_keep_cnt, int64_t cap)
{
    return vdet_nms_volume_topk(c, d_boxes, d_scores, layout, F, B, C, thresh, use_score_thresh, score_thresh, 0,
                                d_keep_idx, d_keep_cnt, cap);
}

int vdet_nms_volume_topk(vdet_ctx *c, const float *d_boxes, const float *d_scores, int layout, int64_t F, int64_t B,
                         int64_t C, double thresh, int use_score_thresh, float score_thresh, int topk,
                         int32_t *d_keep_idx, int32_t *d_keep_cnt, int64_t cap)
{
    if (!c) return VDET_EINVAL;
    if (F < 0 || B < 0 || C < 0 || cap < 0 || topk < 0 || (layout != VDET_LAYOUT_FBC && layout != VDET_LAYOUT_FCB))
        return fail(c, VDET_EINVAL, "bad shape/layout");
    if (F == 0 || C == 0) return VDET_OK;
    if (!d_keep_cnt || (cap > 0 && !d_keep_idx)) return fail(c, VDET_EINVAL, "null output");
    int rc = check_volume(c, d_boxes, F, B, C);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    if (B == 0) {
        HIPCHK(c, hipMemsetAsync(d_keep_cnt, 0, (size_t)(F * C) * 4, c->stream));
        return VDET_OK;
    }
    bool same_geo = false;
    if ((rc = ensure_volume_graph(c, d_boxes, F, B, thresh, true, &same_geo))) return rc;
    const ListsKey key{d_scores, C, layout, use_score_thresh, score_thresh, topk};
    SortWalkArgs a{};
    a.walk_only = same_geo && lists_match(c, key, F, B);
    a.mode = layout; a.P = (int)(F * C); a.B = (int)B; a.C = (int)C;
    a.scores = d_scores;
    a.use_thr = use_score_thresh; a.thr = score_thresh; a.topk = topk;
    a.keep_idx = d_keep_idx; a.keep_cnt = d_keep_cnt; a.cap = cap;
    rc = launch_sort_walk(c, a, (int)B, F * C * B);
    if (rc) return rc;
    set_lists(c, key);
    return VDET_OK;
}

// ---------------------------------------------------------------------------------------------
// The Fast R-CNN per-class flow (vdet/video_det.py:89-99 + vdet/image_det.py:117-123): every class suppresses its OWN
// regressed boxes.  Selection (score > thresh, best topk) = the LSD sort's threshold + top-k on the [F,B,K] score
// volume; then one wave per (frame, class) on its <= 128 selected boxes (detnms_kernels.hpp).
// The boxes come from d_boxes [F,B,K,4], or -- dec given -- are decoded at the gather from the head's output (vdet_det_nms_volume_deltas).
struct DetDecodeSrc {
    const void *rois;
    int rois_f64;
    const float *deltas;
    int64_t H, W;
};

static int det_nms_volume_impl(vdet_ctx *c, const float *d_boxes, const DetDecodeSrc *dec, const float *d_scores, int64_t F, int64_t B,
                               int64_t K, int class0, int use_score_thresh, float score_thresh, int topk, double nms_thresh,
                               float *d_dets, int32_t *d_sel_idx, int32_t *d_det_cnt, int32_t *d_keep, int32_t *d_keep_cnt)
{
    if (!c) return VDET_EINVAL;
    if (F < 0 || B < 0 || K < 0 || class0 < 0) return fail(c, VDET_EINVAL, "bad shape");
    if (dec && (dec->H < 1 || dec->W < 1)) return fail(c, VDET_EINVAL, "im_size: H and W must be at least 1");
    if (topk < 1 || topk > kDetMax) return fail(c, VDET_EINVAL, "topk = %d; the per-class NMS takes 1..%d boxes per (frame, class)", topk, kDetMax);
    if (F == 0 || K == 0) return VDET_OK;
    if (!d_det_cnt || !d_keep || !d_keep_cnt) return fail(c, VDET_EINVAL, "null output");
    if (B > 32767) return fail(c, VDET_EINVAL, "B = %lld boxes per frame; the limit is 32767", (long long)B);
    if (!fits_upto(0x7FFFFFF0ll, {F, K}) || !fits_upto(0x7FFFFFF0ll, {F, B})) return fail(c, VDET_EINVAL, "volume too large");
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    if (B == 0) {
        HIPCHK(c, hipMemsetAsync(d_det_cnt, 0, (size_t)(F * K) * 4, c->stream));
        HIPCHK(c, hipMemsetAsync(d_keep_cnt, 0, (size_t)(F * K) * 4, c->stream));
        return VDET_OK;
    }
    if (dec) {
        if (!dec->rois || !dec->deltas || !d_scores) return fail(c, VDET_EINVAL, "null buffer");
        if ((((uintptr_t)dec->rois | (uintptr_t)dec->deltas) & 15) != 0) return fail(c, VDET_EINVAL, "d_rois and d_deltas must be 16-byte aligned");
    } else {
        if (!d_boxes || !d_scores) return fail(c, VDET_EINVAL, "null buffer");
        if (((uintptr_t)d_boxes & 15) != 0) return fail(c, VDET_EINVAL, "d_boxes must be 16-byte aligned");
    }
    // (no suppression graph is shared between classes here)
    int rc = volume_groups(c, F, B);
    if (rc) return rc;
    c->lists_valid = false;          // (the context's lists become the selections)
    HIPCHK(c, c->nover.reserve((size_t)(F * K) * 4));
    SortWalkArgs a = volume_sort_args(F, B, K, d_scores);
    a.use_thr = use_score_thresh ? 1 : 0; a.thr = score_thresh; a.topk = topk;
    a.nover_out = c->nover.as<int32_t>();
    if ((rc = launch_sort_walk(c, a, (int)B, F * K * B))) return rc;
    DetNmsParams dp{};
    dp.boxes = reinterpret_cast<const float4 *>(d_boxes); dp.scores = d_scores;
    dp.F = (int)F; dp.B = (int)B; dp.K = (int)K; dp.class0 = class0;
    dp.order = c->order.as<uint16_t>(); dp.ncand = c->ncand.as<int32_t>(); dp.nover = c->nover.as<int32_t>();
    dp.topk = topk; dp.t32 = thresh_to_f32(nms_thresh);
    dp.dets = d_dets; dp.sel_idx = d_sel_idx; dp.det_cnt = d_det_cnt; dp.keep = d_keep; dp.keep_cnt = d_keep_cnt;
    dp.status = &c->d_cnt->status;
    {
        StageTimer tm(c, ST_WALK);
        const dim3 grid((unsigned)((F * K + 3) / 4));
        if (!dec) {
            hipLaunchKernelGGL(det_nms_kernel, grid, dim3(256), 0, c->stream, dp);
        } else if (dec->rois_f64) {
            const DetBoxFromDeltas<true> src{dec->rois, reinterpret_cast<const float4 *>(dec->deltas), (int)B, (double)(dec->W - 1), (double)(dec->H - 1)};
            hipLaunchKernelGGL(det_nms_deltas_kernel<true>, grid, dim3(256), 0, c->stream, dp, src);
        } else {
            const DetBoxFromDeltas<false> src{dec->rois, reinterpret_cast<const float4 *>(dec->deltas), (int)B, (double)(dec->W - 1), (double)(dec->H - 1)};
            hipLaunchKernelGGL(det_nms_deltas_kernel<false>, grid, dim3(256), 0, c->stream, dp, src);
        }
    }
    HIPCHK(c, hipGetLastError());
    return VDET_OK;
}

int vdet_det_nms_volume(vdet_ctx *c, const float *d_boxes, const float *d_scores, int64_t F, int64_t B, int64_t K, int class0,
                        int use_score_thresh, float score_thresh, int topk, double nms_thresh, float *d_dets, int32_t *d_sel_idx,
                        int32_t *d_det_cnt, int32_t *d_keep, int32_t *d_keep_cnt)
{
    return det_nms_volume_impl(c, d_boxes, nullptr, d_scores, F, B, K, class0, use_score_thresh, score_thresh, topk, nms_thresh, d_dets,
                               d_sel_idx, d_det_cnt, d_keep, d_keep_cnt);
}

// ---------------------------------------------------------------------------------------------
// The box decode of the Fast R-CNN route (decode_kernels.hpp; THE rule: tests/decode_spec.py)
static int decode_size_check(vdet_ctx *c, int64_t H, int64_t W)
{
    if (H < 1 || W < 1) return fail(c, VDET_EINVAL, "im_size: H and W must be at least 1");
    return VDET_OK;
}

int vdet_decode_boxes(vdet_ctx *c, const void *d_rois, int rois_f64, const float *d_deltas, int64_t N, int64_t K, int64_t H, int64_t W,
                      float *d_boxes)
{
    if (!c) return VDET_EINVAL;
    if (N < 0 || K < 0 || K > 0x7FFFFFF0ll) return fail(c, VDET_EINVAL, "bad shape");
    if (decode_size_check(c, H, W)) return VDET_EINVAL;
    if (N == 0 || K == 0) return VDET_OK;
    if (!fits_upto(1ll << 40, {N, K})) return fail(c, VDET_EINVAL, "too many boxes for one launch (N*K up to 2^40)");
    if (!d_rois || !d_deltas || !d_boxes) return fail(c, VDET_EINVAL, "null buffer");
    if ((((uintptr_t)d_rois | (uintptr_t)d_deltas | (uintptr_t)d_boxes) & 15) != 0)
        return fail(c, VDET_EINVAL, "d_rois, d_deltas and d_boxes must be 16-byte aligned");
    const int64_t blocks = (N * K + 255) / 256;
    if (blocks > 0x7FFFFFFFll) return fail(c, VDET_EINVAL, "too many boxes for one launch");
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    DecodeArgs a{};
    a.rois = d_rois; a.deltas = reinterpret_cast<const float4 *>(d_deltas); a.N = N; a.K = (int)K;
    a.wmax = (double)(W - 1); a.hmax = (double)(H - 1);
    a.boxes = reinterpret_cast<float4 *>(d_boxes);
    {
        StageTimer tm(c, ST_OTHER);
        if (rois_f64) hipLaunchKernelGGL(decode_boxes_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, c->stream, a);
        else hipLaunchKernelGGL(decode_boxes_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, c->stream, a);
    }
    HIPCHK(c, hipGetLastError());
    return VDET_OK;
}

int vdet_det_nms_volume_deltas(vdet_ctx *c, const void *d_rois, int rois_f64, const float *d_scores, const float *d_deltas, int64_t F,
                               int64_t B, int64_t K, int64_t H, int64_t W, int class0, int use_score_thresh, float score_thresh,
                               int topk, double nms_thresh, float *d_dets, int32_t *d_sel_idx, int32_t *d_det_cnt, int32_t *d_keep,
                               int32_t *d_keep_cnt)
{
    const DetDecodeSrc dec{d_rois, rois_f64, d_deltas, H, W};
    return det_nms_volume_impl(c, nullptr, &dec, d_scores, F, B, K, class0, use_score_thresh, score_thresh, topk, nms_thresh, d_dets,
                               d_sel_idx, d_det_cnt, d_keep, d_keep_cnt);
}

int vdet_tubelet_dets(vdet_ctx *c, const float *d_scores, const float *d_deltas, int64_t N, int64_t K, const void *d_tracks,
                      int tracks_f64, int ld, const int32_t *d_slot, const int32_t *d_count, int64_t C, int T, int64_t F,
                      const int32_t *d_cols, int64_t H, int64_t W, double *d_det, float *d_tboxes)
{
    if (!c) return VDET_EINVAL;
    if (N < 0 || K < 1 || K > 0x7FFFFFF0ll || ld < 4) return fail(c, VDET_EINVAL, "bad shape (N >= 0 rows, K >= 1 columns, ld >= 4)");
    if (decode_size_check(c, H, W)) return VDET_EINVAL;
    if (C < 1 || T < 1 || F < 1 || !fits_below(0x7FFFFFF0ll, {C, T, F}))
        return fail(c, VDET_EINVAL, "shape must be C, T, F >= 1 with C*T*F below 2^31 - 16");
    if (N == 0) return VDET_OK;
    if (!fits_upto(1ll << 40, {N, K})) return fail(c, VDET_EINVAL, "too many rows (N*K up to 2^40)");
    if (!d_scores || !d_deltas || !d_tracks || !d_slot || !d_det || !d_tboxes) return fail(c, VDET_EINVAL, "null buffer");
    if ((((uintptr_t)d_deltas | (uintptr_t)d_tboxes) & 15) != 0) return fail(c, VDET_EINVAL, "d_deltas and d_tboxes must be 16-byte aligned");
    const int64_t blocks = (N + 255) / 256;
    if (blocks > 0x7FFFFFFFll) return fail(c, VDET_EINVAL, "too many rows for one launch");
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    TubeletDetsArgs a{};
    a.scores = d_scores; a.deltas = reinterpret_cast<const float4 *>(d_deltas); a.tracks = d_tracks; a.ld = ld;
    a.slot = d_slot; a.count = d_count; a.cols = d_cols; a.N = N; a.K = (int)K; a.C = C; a.F = F; a.T = T;
    a.wmax = (double)(W - 1); a.hmax = (double)(H - 1);
    a.det = d_det; a.tboxes = reinterpret_cast<float4 *>(d_tboxes); a.status = &c->d_cnt->status;
    {
        StageTimer tm(c, ST_OTHER);
        if (tracks_f64) hipLaunchKernelGGL(tubelet_dets_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, c->stream, a);
        else hipLaunchKernelGGL(tubelet_dets_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, c->stream, a);
    }
    HIPCHK(c, hipGetLastError());
    return VDET_OK;
}

int vdet_dets_as_tracks(vdet_ctx *c, const float *d_dets, const int32_t *d_sel_idx, const int32_t *d_keep, const int32_t *d_keep_cnt,
                        int64_t F, int64_t K, int topk, int class0, float *d_tracks, double *d_score, int32_t *d_src, int32_t *d_cnt,
                        int32_t *d_ntracks)
{
    if (!c) return VDET_EINVAL;
    if (F < 1 || K < 1 || class0 < 0 || class0 >= K) return fail(c, VDET_EINVAL, "bad shape (F >= 1 frames, K >= 1 classes, 0 <= first_class < K)");
    if (topk < 1 || topk > kDetMax) return fail(c, VDET_EINVAL, "topk = %d; the per-class NMS takes 1..%d boxes per (frame, class)", topk, kDetMax);
    if (!fits_below(0x7FFFFFF0ll, {K, (int64_t)topk, F})) return fail(c, VDET_EINVAL, "volume too large (K*topk*F must stay below 2^31 - 16)");
    if (!d_dets || !d_sel_idx || !d_keep || !d_keep_cnt || !d_tracks || !d_score || !d_src || !d_cnt || !d_ntracks)
        return fail(c, VDET_EINVAL, "null buffer");
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    const int64_t C = K - class0;
    DetsAsTracksArgs a{};
    a.dets = d_dets; a.sel_idx = d_sel_idx; a.keep = d_keep; a.keep_cnt = d_keep_cnt;
    a.F = F; a.K = (int)K; a.class0 = class0; a.R = topk;
    a.tracks = d_tracks; a.score = d_score; a.src = d_src; a.cnt = d_cnt; a.ntracks = d_ntracks;
    HIPCHK(c, hipMemsetAsync(d_ntracks, 0, (size_t)C * 4, c->stream));
    {
        StageTimer tm(c, ST_OTHER);
        hipLaunchKernelGGL(dets_as_tracks_kernel, dim3((unsigned)((C * topk * F + 255) / 256)), dim3(256), 0, c->stream, a);
    }
    HIPCHK(c, hipGetLastError());
    return VDET_OK;
}

// ---------------------------------------------------------------------------------------------
// (inner: a stage of another entry point, whose stage timers stay)
static int nms_volume_ordered_impl(vdet_ctx *c, const float *d_boxes, const uint16_t *d_order, const int32_t *d_ncand, int64_t F, int64_t B,
                                   int64_t C, double thresh, int32_t *d_keep_idx, int32_t *d_keep_cnt, int64_t cap, bool inner)
{
    if (!c) return VDET_EINVAL;
    if (F < 0 || B < 0 || C < 0 || cap < 0) return fail(c, VDET_EINVAL, "bad shape");
    if (F == 0 || C == 0) return VDET_OK;
    if (!d_keep_cnt || (cap > 0 && !d_keep_idx)) return fail(c, VDET_EINVAL, "null output");
    if (B > 32767) return fail(c, VDET_EINVAL, "B = %lld boxes per frame; the limit is 32767", (long long)B);
    if (!fits_upto(0x7FFFFFF0ll, {F, C}) || !fits_upto(0x7FFFFFF0ll, {F, B})) return fail(c, VDET_EINVAL, "volume too large");
    HIPCHK(c, hipSetDevice(c->device));
    if (!inner) timing_reset(c);
    if (B == 0) {
        HIPCHK(c, hipMemsetAsync(d_keep_cnt, 0, (size_t)(F * C) * 4, c->stream));
        return VDET_OK;
    }
    if (!d_boxes || !d_order || !d_ncand) return fail(c, VDET_EINVAL, "null buffer");
    if (((uintptr_t)d_boxes & 15) != 0) return fail(c, VDET_EINVAL, "d_boxes must be 16-byte aligned");
    const int rc = ensure_volume_graph(c, d_boxes, F, B, thresh, true);
    if (rc) return rc;
    // the lists are the caller's: counts / indices out of range latch VDET_EINVAL (vdet_sync) and the list is walked as empty
    HIPCHK(c, c->ordncand.reserve((size_t)(F * C) * 4));
    hipLaunchKernelGGL(check_order_kernel, dim3((unsigned)((F * C + 3) / 4)), dim3(256), 0, c->stream, d_order, d_ncand, (int)(F * C), (int)B,
                       c->ordncand.as<int32_t>(), &c->d_cnt->status);
    SortWalkArgs a{};
    a.walk_only = true;
    a.mode = 1; a.P = (int)(F * C); a.B = (int)B; a.C = (int)C;
    a.order_in = d_order; a.ncand_in = c->ordncand.as<int32_t>();
    a.keep_idx = d_keep_idx; a.keep_cnt = d_keep_cnt; a.cap = cap;
    return launch_sort_walk(c, a, (int)B, F * C * B);
}

int vdet_nms_volume_ordered(vdet_ctx *c, const float *d_boxes, const uint16_t *d_order, const int32_t *d_ncand, int64_t F, int64_t B,
                            int64_t C, double thresh, int32_t *d_keep_idx, int32_t *d_keep_cnt, int64_t cap)
{
    return nms_volume_ordered_impl(c, d_boxes, d_order, d_ncand, F, B, C, thresh, d_keep_idx, d_keep_cnt, cap, false);
}

// ---------------------------------------------------------------------------------------------
// The proposal layer of a region proposal network (proposal_kernels.hpp; THE rule: tests/rpn_spec.py): decode + keys, per-frame
// select + sort, the ordered-list NMS over the candidates (one list per frame, identity order), gather.
int vdet_rpn_proposals(vdet_ctx *c, const float *d_scores, int64_t score_frame_stride, const float *d_deltas, const double *d_anchors,
                       int64_t F, int64_t A, int64_t Hf, int64_t Wf, int64_t H, int64_t W, int64_t stride, int64_t pre_nms_top_n,
                       int64_t post_nms_top_n, double nms_thresh, double min_size, double offset, int use_dw_max, double dw_max,
                       float *d_rois, float *d_out_scores, int32_t *d_index, int32_t *d_count, int32_t *d_cand_index,
                       int32_t *d_cand_cnt)
{
    if (!c) return VDET_EINVAL;
    if (F < 0) return fail(c, VDET_EINVAL, "bad shape");
    if (A < 1 || A > kRpnMaxA) return fail(c, VDET_EINVAL, "A = %lld anchors per cell; 1 .. %d", (long long)A, kRpnMaxA);
    if (Hf < 1 || Wf < 1 || !fits_below(1ll << 24, {Hf, Wf, A}))
        return fail(c, VDET_EINVAL, "the feature map must be Hf, Wf >= 1 with Hf*Wf*A below 2^24");
    const int64_t N = Hf * Wf * A;
    if (!fits_below(0x7FFFFFF0ll, {F, N})) return fail(c, VDET_EINVAL, "volume too large (F*Hf*Wf*A must stay below 2^31 - 16)");
    if (stride < 1 || stride > 0x7FFFFFFFll) return fail(c, VDET_EINVAL, "stride must be an integer >= 1");
    if (post_nms_top_n < 1 || post_nms_top_n > pre_nms_top_n || pre_nms_top_n > kRpnMaxPre)
        return fail(c, VDET_EINVAL, "1 <= post_nms_top_n <= pre_nms_top_n <= %d", kRpnMaxPre);
    if (!fits_below(0x7FFFFFF0ll, {F, pre_nms_top_n})) return fail(c, VDET_EINVAL, "volume too large (F*pre_nms_top_n must stay below 2^31 - 16)");
    if (decode_size_check(c, H, W)) return VDET_EINVAL;
    if (!std::isfinite(min_size) || !std::isfinite(offset)) return fail(c, VDET_EINVAL, "min_size and offset must be finite");
    if (use_dw_max && dw_max != dw_max) return fail(c, VDET_EINVAL, "dw_max must not be NaN");
    if (score_frame_stride < N) return fail(c, VDET_EINVAL, "the scores' frame stride must be at least A*Hf*Wf elements");
    if (F == 0) return VDET_OK;
    if (!d_scores || !d_deltas || !d_anchors || !d_rois || !d_out_scores || !d_index || !d_count) return fail(c, VDET_EINVAL, "null buffer");
    if (((uintptr_t)d_rois & 15) != 0) return fail(c, VDET_EINVAL, "d_rois must be 16-byte aligned");
    const int pre = (int)pre_nms_top_n, post = (int)post_nms_top_n;
    int p2 = 1;
    while (p2 < pre) p2 <<= 1;
    const size_t sel_lds = (size_t)p2 * 8;
    if (sel_lds + 4096 > c->max_lds) return fail(c, VDET_EINVAL, "pre_nms_top_n = %d needs %zu B of LDS for the in-LDS sort", pre, sel_lds);
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    if (!c->rpn_attr_set) {
        HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void *>(rpn_select_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)std::min<size_t>((size_t)kRpnMaxPre * 8, c->max_lds - 4096)));
        c->rpn_attr_set = true;
    }
    HIPCHK(c, c->rpn_keys.reserve((size_t)(F * N) * 4));
    HIPCHK(c, c->rpn_boxes.reserve((size_t)(F * N) * 16));
    HIPCHK(c, c->rpn_cbox.reserve((size_t)(F * pre) * 16));
    HIPCHK(c, c->rpn_cscore.reserve((size_t)(F * pre) * 4));
    HIPCHK(c, c->rpn_order.reserve((size_t)(F * pre) * 2));
    HIPCHK(c, c->rpn_keep.reserve((size_t)(F * pre) * 4));
    HIPCHK(c, c->rpn_keepcnt.reserve((size_t)F * 4));
    if (!d_cand_index) { HIPCHK(c, c->rpn_cindex.reserve((size_t)(F * pre) * 4)); d_cand_index = c->rpn_cindex.as<int32_t>(); }
    if (!d_cand_cnt) { HIPCHK(c, c->rpn_ccnt.reserve((size_t)F * 4)); d_cand_cnt = c->rpn_ccnt.as<int32_t>(); }

    RpnDecodeArgs da{};
    da.scores = d_scores; da.sstride = score_frame_stride; da.deltas = d_deltas; da.anchors = d_anchors;
    da.A = (int)A; da.Hf = (int)Hf; da.Wf = (int)Wf; da.wtiles = (int)((Wf + 63) / 64); da.N = N;
    da.stride = (double)stride; da.wmax = (double)(W - 1); da.hmax = (double)(H - 1); da.min_size = min_size; da.offset = offset;
    da.use_dw_max = use_dw_max ? 1 : 0; da.dw_max = use_dw_max ? dw_max : 0.0;
    da.keys = c->rpn_keys.as<uint32_t>(); da.boxes = c->rpn_boxes.as<float4>();
    RpnSelectArgs sa{};
    sa.keys = da.keys; sa.boxes = da.boxes; sa.scores = d_scores; sa.sstride = score_frame_stride; sa.A = (int)A; sa.HW = Hf * Wf; sa.N = N;
    sa.pre = pre; sa.p2 = p2;
    sa.cand_boxes = c->rpn_cbox.as<float4>(); sa.cand_scores = c->rpn_cscore.as<float>(); sa.cand_index = d_cand_index;
    sa.order = c->rpn_order.as<uint16_t>(); sa.cand_cnt = d_cand_cnt;
    {
        StageTimer tm(c, ST_OTHER);
        hipLaunchKernelGGL(rpn_decode_kernel, dim3((unsigned)(F * Hf * da.wtiles)), dim3(256), 0, c->stream, da);
    }
    {
        StageTimer tm(c, ST_SORT);
        hipLaunchKernelGGL(rpn_select_kernel, dim3((unsigned)F), dim3(kRpnSelBlock), sel_lds, c->stream, sa);
    }
    HIPCHK(c, hipGetLastError());
    // the candidates are the context's own scratch: a resident graph keyed on that address describes the call before
    c->graph_valid = false;
    const int rc = nms_volume_ordered_impl(c, c->rpn_cbox.as<float>(), sa.order, d_cand_cnt, F, pre, 1, nms_thresh, c->rpn_keep.as<int32_t>(),
                                           c->rpn_keepcnt.as<int32_t>(), pre, true);      // (cap = pre: the cut at post is the gather's, no VDET_ECAP)
    c->graph_valid = false;
    if (rc) return rc;
    RpnGatherArgs ga{};
    ga.cand_boxes = sa.cand_boxes; ga.cand_scores = sa.cand_scores; ga.cand_index = d_cand_index;
    ga.keep = c->rpn_keep.as<int32_t>(); ga.keep_cnt = c->rpn_keepcnt.as<int32_t>();
    ga.F = F; ga.pre = pre; ga.post = post;
    ga.rois = reinterpret_cast<float4 *>(d_rois); ga.scores = d_out_scores; ga.index = d_index; ga.count = d_count;
    {
        StageTimer tm(c, ST_OTHER);
        hipLaunchKernelGGL(rpn_gather_kernel, dim3((unsigned)((F * post + 255) / 256)), dim3(256), 0, c->stream, ga);
    }
    HIPCHK(c, hipGetLastError());
    return VDET_OK;
}

// ---------------------------------------------------------------------------------------------
int vdet_argsort_volume(vdet_ctx *c, const float *d_scores, int layout, int64_t F, int64_t B, int64_t C,
                        int use_score_thresh, float score_thresh, uint16_t *d_order, int32_t *d_ncand)
{
    if (!c) return VDET_EINVAL;
    if (F < 0 || B < 0 || C < 0 || (layout != VDET_LAYOUT_FBC && layout != VDET_LAYOUT_FCB)) return fail(c, VDET_EINVAL, "bad shape/layout");
    if (F == 0 || C == 0) return VDET_OK;
    if (!d_ncand || (B > 0 && (!d_scores || !d_order))) return fail(c, VDET_EINVAL, "null buffer");
    if (B > 32767) return fail(c, VDET_EINVAL, "B = %lld boxes per frame; the limit is 32767", (long long)B);
    if (!fits_upto(0x7FFFFFF0ll, {F, C}) || !fits_upto(0x7FFFFFF0ll, {F, B})) return fail(c, VDET_EINVAL, "volume too large");
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    if (B == 0) {
        HIPCHK(c, hipMemsetAsync(d_ncand, 0, (size_t)(F * C) * 4, c->stream));
        return VDET_OK;
    }
    const int rc = volume_groups(c, F, B);
    if (rc) return rc;
    c->lists_valid = false;          // (c->tkeys, which the context's own lists are read with, is rewritten)
    SortWalkArgs a{};
    a.sort_only = true;
    a.mode = layout; a.P = (int)(F * C); a.B = (int)B; a.C = (int)C;
    a.scores = d_scores;
    a.use_thr = use_score_thresh; a.thr = score_thresh;
    a.order_out = d_order; a.ncand_out = d_ncand;
    return launch_sort_walk(c, a, (int)B, F * C * B);
}

// ---------------------------------------------------------------------------------------------
int vdet_track_volume(vdet_ctx *c, const float *d_boxes, const float *d_scores, int64_t F, int64_t B, int64_t C,
                      double nms_thres, double thres, int max_tracks, double link_thres, int max_frames,
                      float *d_tracks, float *d_anchors, int32_t *d_ntracks)
{
    return vdet_nms_track_volume(c, d_boxes, d_scores, F, B, C, nms_thres, thres, max_tracks, link_thres, max_frames,
                                 d_tracks, d_anchors, d_ntracks, 0, nullptr, nullptr);
}

int vdet_nms_track_volume(vdet_ctx *c, const float *d_boxes, const float *d_scores, int64_t F, int64_t B, int64_t C,
                          double nms_thres, double thres, int max_tracks, double link_thres, int max_frames,
                          float *d_tracks, float *d_anchors, int32_t *d_ntracks, int64_t cap, int32_t *d_keep_idx,
                          int32_t *d_keep_cnt)
{
    if (!c) return VDET_EINVAL;
    const bool want_nms = d_keep_cnt != nullptr;
    if (want_nms && (cap < 0 || (cap > 0 && !d_keep_idx))) return fail(c, VDET_EINVAL, "null output");
    if (F <= 0 || B <= 0 || C <= 0 || max_tracks < 0) return fail(c, VDET_EINVAL, "bad shape");
    if (!d_boxes || !d_scores || !d_ntracks || (max_tracks > 0 && (!d_tracks || !d_anchors)))
        return fail(c, VDET_EINVAL, "null buffer");
    int rc = check_volume(c, d_boxes, F, B, C);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    if ((rc = volume_lists(c, d_boxes, d_scores, F, B, C, nms_thres, true))) return rc;
    // regular-frame fast paths (lazy lists, x-window link): only when THIS graph build (or the cached
    // one being reused) ran K0 + the frame index -- gflags / the index are stale otherwise
    const TrackWork w = track_work(c, B, link_thres, max_frames, (int)F);
    // small frames (filled): the whole link table up front (every node's window scan, chip-filling) -- then no step of any
    // chain is ever scanned again, whatever the anchors turn out to be.
    // Warm the memo otherwise: the chains of every class's likely anchors, all at once (the chip is full instead of
    // running 2 C latency-bound blocks per track); the tracking loop below then mostly walks known steps.  + slots for
    // the anchors of COHERENT videos (track_warm_anchors_body: filled only when a class's raw candidates repeat each
    // other's objects across frames; empty -- and free -- otherwise)
    const int wm_raw = std::min(max_tracks + 6, 24);       // (measured: 16 of 10 tracks)
    const bool coherent_slots = F <= 512 && w.flags && !w.filled;
    const int wm = coherent_slots ? std::min(wm_raw + max_tracks, 32) : wm_raw;
    if ((rc = track_scratch(c, F, B, C, max_tracks, wm, C))) return rc;
    int materialized = 0;            // warm chains per class whose tubelets are written out (0: none)
    if (max_tracks > 0) {
        StageTimer tm(c, ST_TLINK);
        if (w.filled)
            hipLaunchKernelGGL(link_fill_frame_kernel, dim3((unsigned)F, 2), dim3((unsigned)(64 * ((B + 63) / 64))), link_fill_lds_bytes((int)B), c->stream,
                               reinterpret_cast<const float4 *>(d_boxes), (int)F, (int)B, w.link_t32, w.flags, w.ix, link_thres,
                               c->linkmemo.as<unsigned long long>());
        hipLaunchKernelGGL(track_warm_anchors_kernel, dim3((unsigned)C), dim3(256), 0, c->stream, c->tkeys.as<uint32_t>(),
                           c->order.as<uint16_t>(), c->ncand.as<int32_t>(), (int)F, (int)B, (int)C, d_scores, thres, wm,
                           c->linkwarm.as<int32_t>(),
                           WarmExtra{coherent_slots ? reinterpret_cast<const float4 *>(d_boxes) : nullptr, thresh_to_f32(nms_thres), wm_raw,
                                     max_tracks});
        if (!w.filled) {
            // longest chains first, then every (chain, direction) as one block of the warm-up launch
            HIPCHK(c, c->linkorder.reserve((size_t)C * wm * 2 * 4));
            hipLaunchKernelGGL(warm_order_kernel, dim3(1), dim3(1024), 0, c->stream, c->linkwarm.as<int32_t>(), (int)(C * wm), (int)F, (int)B,
                               w.reach, c->linkorder.as<int32_t>());
            hipLaunchKernelGGL((track_link_memo_kernel<256, 1, 8>), dim3((unsigned)(C * wm), 2), dim3(256), 0, c->stream,
                               reinterpret_cast<const float4 *>(d_boxes), (int)F, (int)B, max_tracks, w.link_t32, w.reach,
                               (const TrackState *)nullptr, (float *)nullptr, w.flags, w.ix, link_thres,
                               c->linkmemo.as<unsigned long long>(), c->linkstats.as<unsigned int>(), c->linkwarm.as<int32_t>(),
                               (int32_t *)nullptr, (const int32_t *)c->linkorder.as<int32_t>());
        }
        // every step of the warm chains is known now: write each predicted anchor's tubelet ONCE (one wave walks a chain; all
        // of them side by side), for the tracking loop to copy
        hipLaunchKernelGGL((track_link_memo_kernel<64, 2, 8>), dim3((unsigned)(C * wm), 2), dim3(64), 0, c->stream,
                           reinterpret_cast<const float4 *>(d_boxes), (int)F, (int)B, max_tracks, w.link_t32, w.reach,
                           (const TrackState *)nullptr, c->linkchains.as<float>(), w.flags, w.ix, link_thres,
                           c->linkmemo.as<unsigned long long>(), (unsigned int *)nullptr, c->linkwarm.as<int32_t>(),
                           c->linknodes.as<int32_t>(), (const int32_t *)nullptr);
        materialized = wm;
    }
    // the NMS survivors: one walk over the lists, before they are consumed
    if (want_nms && (rc = launch_sort_walk(c, volume_walk_args(F, B, C, d_scores, d_keep_idx, d_keep_cnt, cap), (int)B, F * C * B))) return rc;
    if ((rc = track_begin(c, C, max_tracks, d_ntracks)) || max_tracks == 0) return rc;
    GreedyArgs g = greedy_args(c, w, d_boxes, d_scores, F, B, C, nms_thres, thres, max_tracks, d_tracks, d_anchors, d_ntracks);
    LoopArgs &la = g.la;            // the link fields
    la.link_thres = link_thres; la.link_t32 = w.link_t32; la.reach = w.reach;
    la.memo = c->linkmemo.as<unsigned long long>(); la.stats = c->linkstats.as<unsigned int>();
    la.nodes = c->tracknode.as<int32_t>();
    // predicted anchors: their tubelets exist already, the loop copies them
    ResolveArgs rv{c->linkwarm.as<int32_t>(), materialized, c->linkchains.as<float>(), c->linknodes.as<int32_t>(), d_tracks,
                   c->tracknode.as<int32_t>()};
    {
        // the whole tracking loop in one launch: one persistent block per class (track_loop_kernel)
        StageTimer tm(c, ST_TLOOP);
        hipLaunchKernelGGL(track_loop_kernel, dim3((unsigned)C), dim3(256), (size_t)w.mask_words * 16, c->stream, la, g.lz, rv, g.sp);
    }
    HIPCHK(c, hipGetLastError());
    c->nodekey.tracks = d_tracks; c->nodekey.boxes = d_boxes; c->nodekey.F = F; c->nodekey.B = B; c->nodekey.C = C;
    c->nodekey.T = max_tracks; c->nodekey.nms_thres = nms_thres;
    c->nodes_valid = true;
    return VDET_OK;
}

// ---------------------------------------------------------------------------------------------
// V small videos in one call (BASELINE configs[0] / [4] shapes: hundreds of frames x <= 300 boxes x 30 classes, where
// one video alone is launch-bound at ~60 launches): the frames of all videos are concatenated along F -- per-frame NMS
// problems do not know which video they belong to, so suppression graph, sort and walk are ONE launch sequence for the
// whole batch -- and only the stages that follow a video in time (tracking, re-scoring) run per video, on sub-ranges
// of the same buffers, with the video as a grid dimension (batch_kernels.hpp): one launch per stage for all videos instead of
// ~60 launches per video, no host synchronisation in between.
// ---------------------------------------------------------------------------------------------
int vdet_video_batch(vdet_ctx *c, const float *d_boxes, const float *d_scores, const int64_t *h_frame_off, int64_t V, int64_t B,
                     int64_t C, double nms_thres, double thres, int max_tracks, double link_thres, int max_frames,
                     float *d_tracks, float *d_anchors, int32_t *d_ntracks, int64_t cap, int32_t *d_keep_idx, int32_t *d_keep_cnt,
                     double overlap_thres, int window, double *d_det_score, double *d_pooled, float *d_boxes_out)
{
    if (!c) return VDET_EINVAL;
    const bool want_nms = d_keep_cnt != nullptr, want_rescore = d_pooled != nullptr;
    if (want_nms && (cap < 0 || (cap > 0 && !d_keep_idx))) return fail(c, VDET_EINVAL, "null output");
    if (B <= 0 || C <= 0 || max_tracks < 0) return fail(c, VDET_EINVAL, "bad shape");
    if (!d_boxes || !d_scores || !d_ntracks || (max_tracks > 0 && (!d_tracks || !d_anchors))) return fail(c, VDET_EINVAL, "null buffer");
    if (want_rescore && (!d_det_score || !d_boxes_out)) return fail(c, VDET_EINVAL, "null buffer");
    if (want_rescore && (window < 1 || window % 2 != 1)) return fail(c, VDET_EINVAL, "Window size must be odd!");
    if (B > 32767) return fail(c, VDET_EINVAL, "B = %lld boxes per frame; the limit is 32767", (long long)B);
    if (((uintptr_t)d_boxes & 15) != 0) return fail(c, VDET_EINVAL, "d_boxes must be 16-byte aligned");
    Videos vs;
    int rc = read_videos(c, h_frame_off, V, 0, &vs);
    if (rc) return rc;
    const int64_t F = vs.F, Fmax = vs.Fmax;
    if (!fits_upto(0x7FFFFFF0ll, {F, C}) || !fits_upto(0x7FFFFFF0ll, {F, B}) || !fits_upto(0x7FFFFFF0ll, {V, C})) return fail(c, VDET_EINVAL, "volume too large");
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    const float t32 = thresh_to_f32(nms_thres);
    // ---- the batch as one volume of F frames: graph (always rebuilt), sorted lists, NMS survivors
    if ((rc = volume_lists(c, d_boxes, d_scores, F, B, C, nms_thres, false))) return rc;
    if (want_nms && (rc = launch_sort_walk(c, volume_walk_args(F, B, C, d_scores, d_keep_idx, d_keep_cnt, cap), (int)B, F * C * B))) return rc;
    c->lists_valid = false;          // consumed by the tracking below
    HIPCHK(c, hipMemsetAsync(d_ntracks, 0, (size_t)(V * C) * 4, c->stream));
    if (max_tracks == 0) {
        HIPCHK(c, hipGetLastError());
        return VDET_OK;
    }
    // ---- per video: tracking (+ re-scoring) on its frame range
    const TrackWork w = track_work(c, B, link_thres, max_frames, -1);
    const int T = max_tracks, wm = std::min(T + 6, 24);
    if ((rc = track_scratch(c, F, B, C, T, wm, V * C))) return rc;
    hipLaunchKernelGGL(track_init_kernel, dim3((unsigned)((V * C + 63) / 64)), dim3(64), 0, c->stream, c->tstate.as<TrackState>(), (int)(V * C));
    // ---- all videos side by side: one launch per stage, the video is a grid dimension (batch_kernels.hpp)
    if ((rc = stage_video_table(c, c->vidtab, vs))) return rc;
    BatchTrack bt{};
    bt.vids = c->vidtab.dev.as<VidDesc>();
    bt.Ftot = (int)F; bt.B = (int)B; bt.C = (int)C; bt.T = T; bt.wm = wm;
    bt.boxes = reinterpret_cast<const float4 *>(d_boxes); bt.scores = d_scores;
    bt.keys = c->tkeys.as<uint32_t>(); bt.lists = c->order.as<uint16_t>(); bt.cnt = c->ncand.as<int32_t>();
    bt.group_flags = w.flags; bt.ix = w.ix;
    bt.memo = c->linkmemo.as<unsigned long long>(); bt.stats = c->linkstats.as<unsigned int>();
    bt.warm = c->linkwarm.as<int32_t>(); bt.chains = c->linkchains.as<float>(); bt.chain_nodes = c->linknodes.as<int32_t>();
    bt.track_nodes = c->tracknode.as<int32_t>();
    bt.tracks = d_tracks; bt.anchors = d_anchors; bt.ntracks = d_ntracks;
    bt.st = c->tstate.as<TrackState>();
    bt.heads = c->heads.as<int32_t>(); bt.visited = c->visited.as<uint8_t>();
    bt.groups = c->groups.as<GroupDesc>(); bt.row_meta = c->rowmeta.as<uint2>(); bt.adj = c->adj.as<uint16_t>();
    bt.group_z = c->groupz.as<uint32_t>();
    bt.thres = thres; bt.link_thres = link_thres; bt.nms_thres = nms_thres;
    bt.link_t32 = w.link_t32; bt.t32 = t32; bt.reach_all = w.reach;
    bt.need_suppress = w.need_suppress ? 1 : 0; bt.lazy = w.lazy; bt.mask_words = w.mask_words;
    bt.status = &c->d_cnt->status; bt.n_irregular = &c->d_cnt->irregular;
    {
        StageTimer tm(c, ST_TLINK);
        if (w.filled) {
            // the whole link table of every video: no chain ever scans, whatever its anchor -- so nothing is predicted or
            // materialised either
            hipLaunchKernelGGL(batch_link_fill_frame_kernel, dim3((unsigned)Fmax, 2, (unsigned)V), dim3((unsigned)(64 * ((B + 63) / 64))),
                               link_fill_lds_bytes((int)B), c->stream, bt);
            bt.wm = 0;
        } else {
            hipLaunchKernelGGL(batch_warm_anchors_kernel, dim3((unsigned)C, (unsigned)V), dim3(256), 0, c->stream, bt);
            hipLaunchKernelGGL((batch_link_kernel<256, 1>), dim3((unsigned)(C * wm), 2, (unsigned)V), dim3(256), 0, c->stream, bt);
            hipLaunchKernelGGL((batch_link_kernel<64, 2>), dim3((unsigned)(C * wm), 2, (unsigned)V), dim3(64), 0, c->stream, bt);
        }
    }
    {
        StageTimer tm(c, ST_TLOOP);
        hipLaunchKernelGGL(batch_loop_kernel, dim3((unsigned)C, (unsigned)V), dim3(256), (size_t)w.mask_words * 16, c->stream, bt);
    }
    if (want_rescore) {
        {
            StageTimer tm(c, ST_RSPATIAL);
            // candidates from the suppression graph wherever the tracking loop recorded the proposal a tubelet box came from (as
            // vdet_rescore_tracks does; needs overlap_thres well above the graph's threshold), the window scan for the rest
            const bool use_adj = rescore_from_graph(w.flags, nms_thres, overlap_thres);
            if (use_adj) {
                const int64_t nb = F * C * T;
                HIPCHK(c, c->rtodo.reserve((size_t)nb * 8 + 16));
                unsigned int *cnt = reinterpret_cast<unsigned int *>(c->rtodo.as<char>() + (size_t)nb * 8);
                HIPCHK(c, hipMemsetAsync(cnt, 0, 4, c->stream));
                hipLaunchKernelGGL(batch_rescore_adj_kernel, dim3((unsigned)((Fmax * C * T + 15) / 16), (unsigned)V), dim3(256), 0, c->stream, bt,
                                   overlap_thres, 1.0 - (overlap_thres - nms_thres) + 0.02, d_det_score, d_boxes_out, c->rtodo.as<int2>(), cnt);
                hipLaunchKernelGGL(batch_rescore_todo_kernel, dim3((unsigned)std::min<int64_t>((nb + 3) / 4, 8 * c->n_cu)), dim3(256), 0, c->stream, bt,
                                   overlap_thres, d_det_score, d_boxes_out, c->rtodo.as<int2>(), cnt);
            } else
            hipLaunchKernelGGL(batch_rescore_spatial_kernel, dim3((unsigned)((Fmax * C * T + 3) / 4), (unsigned)V), dim3(256), 0, c->stream, bt,
                               overlap_thres, d_det_score, d_boxes_out);
        }
        StageTimer tm(c, ST_RSERIES);
        // one wave per series with the series in LDS; videos too long for that stage take the one-thread-per-series kernel
        const int stride = (int)(((size_t)std::min<int64_t>(Fmax, kSeriesWaveMaxF) * 9 + 15) & ~(size_t)15);
        hipLaunchKernelGGL(batch_rescore_series_kernel, dim3((unsigned)((C * T + 3) / 4), (unsigned)V), dim3(256), (size_t)stride * 4, c->stream, bt,
                           d_det_score, d_pooled, window, &c->d_cnt->eindex, stride);
        if (Fmax > kSeriesWaveMaxF)
            hipLaunchKernelGGL(batch_rescore_series_long_kernel, dim3((unsigned)((C * T + 63) / 64), (unsigned)V), dim3(64), 0, c->stream, bt,
                               d_det_score, d_pooled, window, &c->d_cnt->eindex);
    }
    HIPCHK(c, hipGetLastError());
    return VDET_OK;
}

int vdet_rescore_tracks(vdet_ctx *c, const float *d_tracks, const int32_t *d_ntracks, const float *d_boxes,
                        const float *d_scores, int64_t F, int64_t B, int64_t C, int max_tracks, double overlap_thres,
                        int window, double *d_det_score, double *d_pooled, float *d_boxes_out)
{
    if (!c) return VDET_EINVAL;
    if (F <= 0 || B <= 0 || C <= 0 || max_tracks < 0) return fail(c, VDET_EINVAL, "bad shape");
    if (window < 1 || window % 2 != 1) return fail(c, VDET_EINVAL, "Window size must be odd!");
    if (max_tracks == 0) return VDET_OK;
    if (!d_tracks || !d_ntracks || !d_boxes || !d_scores || !d_det_score || !d_pooled || !d_boxes_out)
        return fail(c, VDET_EINVAL, "null buffer");
    if (!fits_upto(0x7FFFFFF0ll, {C, max_tracks, F})) return fail(c, VDET_EINVAL, "too many tubelet boxes");
    const int64_t nb = C * max_tracks * F;
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    FrameIndex ix{};
    const uint32_t *flags = nullptr;
    if (!c->no_index && !c->force_general && (size_t)8 * B + 24 * 1024 <= c->max_lds) {   // (the x1 sort must fit the LDS)
        // per-frame regular flags + x-sorted index: reused from the graph build of the same boxes
        // when the cache is on, else rebuilt here (cheap: one 3 M-key sort)
        if (!index_matches(c, d_boxes, F, B)) {
            c->graph_valid = c->lists_valid = c->index_valid = false;       // gflags / the index are rewritten
            int rc = volume_groups(c, F, B);
            if (rc) return rc;
            HIPCHK(c, c->gflags.reserve((size_t)F * 4));
            c->sym_built = false;
            hipLaunchKernelGGL(frame_flags_kernel, dim3((unsigned)F), dim3(256), 0, c->stream,
                               reinterpret_cast<const float4 *>(d_boxes), c->groups.as<GroupDesc>(), c->gflags.as<uint32_t>(),
                               &c->d_cnt->irregular);
            if ((rc = build_frame_index(c, reinterpret_cast<const float4 *>(d_boxes), F * B, F, (int)B))) return rc;
        }
        ix = frame_index_of(c);
        flags = c->gflags.as<uint32_t>();
    }
    {
        StageTimer tm(c, ST_RSPATIAL);
        // the tracks of the last tracking call on this context, same boxes, graph still in place (cache contract):
        // candidates from the suppression graph (see the kernel); needs overlap_thres well above the graph's threshold
        const bool use_adj = nodes_match(c, d_tracks, d_boxes, F, B, C, max_tracks) && rescore_from_graph(flags, c->nodekey.nms_thres, overlap_thres);
        const double min_self = use_adj ? 1.0 - (overlap_thres - c->nodekey.nms_thres) + 0.02 : 2.0;
        const int32_t *todo = nullptr;
        const unsigned int *todo_cnt = nullptr;
        unsigned scan_grid = (unsigned)((nb + 3) / 4);
        if (use_adj) {
            HIPCHK(c, c->rtodo.reserve((size_t)nb * 4 + 16));
            unsigned int *cnt = reinterpret_cast<unsigned int *>(c->rtodo.as<char>() + (size_t)nb * 4);
            HIPCHK(c, hipMemsetAsync(cnt, 0, 4, c->stream));
            hipLaunchKernelGGL(rescore_adj_kernel, dim3((unsigned)((((nb + 15) / 16) + 7) & ~(int64_t)7)), dim3(256), 0, c->stream, d_tracks, d_ntracks,
                               reinterpret_cast<const float4 *>(d_boxes), d_scores, (int)F, (int)B, (int)C, max_tracks,
                               overlap_thres, d_det_score, d_boxes_out, flags, c->tracknode.as<int32_t>(), c->rowmeta.as<uint2>(),
                               c->adj.as<uint16_t>(), min_self, c->rtodo.as<int32_t>(), cnt);
            todo = c->rtodo.as<int32_t>();
            todo_cnt = cnt;
            scan_grid = (unsigned)std::min<int64_t>((nb + 3) / 4, 8 * c->n_cu);
        }
        if (todo)
            hipLaunchKernelGGL(rescore_spatial_kernel<true>, dim3(scan_grid), dim3(256), 0, c->stream, d_tracks, d_ntracks,
                               reinterpret_cast<const float4 *>(d_boxes), d_scores, (int)F, (int)B, (int)C, max_tracks,
                               overlap_thres, d_det_score, d_boxes_out, ix, flags, todo, todo_cnt);
        else
            hipLaunchKernelGGL(rescore_spatial_kernel<false>, dim3(scan_grid), dim3(256), 0, c->stream, d_tracks, d_ntracks,
                               reinterpret_cast<const float4 *>(d_boxes), d_scores, (int)F, (int)B, (int)C, max_tracks,
                               overlap_thres, d_det_score, d_boxes_out, ix, flags, todo, todo_cnt);
    }
    {
        StageTimer tm(c, ST_RSERIES);
        const int n = (int)(C * max_tracks);
        if (F <= kSeriesWaveMaxF) {      // one wave per series, the series in LDS
            const int stride = (int)(((size_t)F * 9 + 15) & ~(size_t)15);
            hipLaunchKernelGGL(rescore_series_wave_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), (size_t)stride * 4, c->stream,
                               d_det_score, d_pooled, d_ntracks, (int)F, (int)C, max_tracks, window, &c->d_cnt->eindex, stride);
        } else {
            hipLaunchKernelGGL(rescore_series_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, c->stream, d_det_score,
                               d_pooled, d_ntracks, (int)F, (int)C, max_tracks, window, &c->d_cnt->eindex);
        }
    }
    HIPCHK(c, hipGetLastError());
    return VDET_OK;
}

// ---------------------------------------------------------------------------------------------
// tubelet re-scoring cores (host buffers)
// ---------------------------------------------------------------------------------------------
static int upload(vdet_ctx *c, DevBuf &b, const void *h, size_t bytes)
{
    HIPCHK(c, b.reserve(std::max<size_t>(bytes, 16)));
    if (bytes) HIPCHK(c, hipMemcpyAsync(b.p, h, bytes, hipMemcpyHostToDevice, c->stream));
    return VDET_OK;
}

static int status_word(vdet_ctx *c, int *out)
{
    Counters h;
    HIPCHK(c, hipMemcpyAsync(&h, c->d_cnt, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, host_sync(c));
    *out = h.status;
    return VDET_OK;
}

int vdet_spatial_maxpool_f64(vdet_ctx *c, const double *h_tub_boxes, const int32_t *h_tub_group, int64_t T,
                             const double *h_det_boxes, const double *h_det_scores, const int64_t *h_group_off,
                             int64_t G, double thres, int64_t *h_out_idx, double *h_out_score)
{
    if (!c || T < 0 || G < 0) return VDET_EINVAL;
    if (T == 0) return VDET_OK;
    if (!h_tub_boxes || !h_tub_group || !h_group_off || !h_out_idx || !h_out_score || G == 0)
        return fail(c, VDET_EINVAL, "null buffer");
    const int64_t M = h_group_off[G];
    for (int64_t t = 0; t < T; ++t)
        if (h_tub_group[t] < 0 || h_tub_group[t] >= G) return fail(c, VDET_EINVAL, "tubelet frame slot out of range");
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    int rc;
    if ((rc = upload(c, c->tmp[0], h_tub_boxes, (size_t)T * 32))) return rc;
    if ((rc = upload(c, c->tmp[1], h_tub_group, (size_t)T * 4))) return rc;
    if ((rc = upload(c, c->tmp[2], h_det_boxes, (size_t)M * 32))) return rc;
    if ((rc = upload(c, c->tmp[3], h_det_scores, (size_t)M * 8))) return rc;
    if ((rc = upload(c, c->tmp[4], h_group_off, (size_t)(G + 1) * 8))) return rc;
    HIPCHK(c, c->tmp[5].reserve((size_t)T * 8));
    HIPCHK(c, c->tmp[6].reserve((size_t)T * 8));
    {
        StageTimer tm(c, ST_OTHER);
        hipLaunchKernelGGL(spatial_maxpool_kernel, dim3((unsigned)T), dim3(256), 0, c->stream, c->tmp[0].as<double>(),
                           c->tmp[1].as<int32_t>(), c->tmp[2].as<double>(), c->tmp[3].as<double>(),
                           c->tmp[4].as<int64_t>(), thres, c->tmp[5].as<int64_t>(), c->tmp[6].as<double>());
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h_out_idx, c->tmp[5].p, (size_t)T * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(h_out_score, c->tmp[6].p, (size_t)T * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, host_sync(c));
    return VDET_OK;
}

int vdet_series_completion_f64(vdet_ctx *c, double *h_vals, const int64_t *h_off, int64_t T)
{
    if (!c || T < 0) return VDET_EINVAL;
    if (T == 0) return VDET_OK;
    if (!h_off) return fail(c, VDET_EINVAL, "null buffer");
    const int64_t n = h_off[T];
    if (n > 0 && !h_vals) return fail(c, VDET_EINVAL, "null buffer");
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    int rc;
    if ((rc = upload(c, c->tmp[0], h_vals, (size_t)n * 8))) return rc;
    if ((rc = upload(c, c->tmp[1], h_off, (size_t)(T + 1) * 8))) return rc;
    HIPCHK(c, hipMemsetAsync(&c->d_cnt->status, 0, sizeof(int), c->stream));
    hipLaunchKernelGGL(series_completion_kernel, dim3((unsigned)((T + 63) / 64)), dim3(64), 0, c->stream,
                       c->tmp[0].as<double>(), c->tmp[1].as<int64_t>(), T, &c->d_cnt->status);
    HIPCHK(c, hipGetLastError());
    if (n) HIPCHK(c, hipMemcpyAsync(h_vals, c->tmp[0].p, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    int st = 0;
    if ((rc = status_word(c, &st))) return rc;
    HIPCHK(c, hipMemsetAsync(&c->d_cnt->status, 0, sizeof(int), c->stream));
    if (st) return fail(c, VDET_EINDEX, "list index out of range");
    return VDET_OK;
}

int vdet_series_maxpool_f64(vdet_ctx *c, const double *h_in, double *h_out, const int64_t *h_off, int64_t T,
                            int window, double pad)
{
    if (!c || T < 0) return VDET_EINVAL;
    if (window < 1 || window % 2 != 1) return fail(c, VDET_EINVAL, "Window size must be odd!");
    if (T == 0) return VDET_OK;
    if (!h_off) return fail(c, VDET_EINVAL, "null buffer");
    const int64_t n = h_off[T];
    if (n == 0) return VDET_OK;
    if (!h_in || !h_out) return fail(c, VDET_EINVAL, "null buffer");
    std::vector<int32_t> es((size_t)n);
    for (int64_t t = 0; t < T; ++t)
        for (int64_t e = h_off[t]; e < h_off[t + 1]; ++e) es[(size_t)e] = (int32_t)t;
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    int rc;
    if ((rc = upload(c, c->tmp[0], h_in, (size_t)n * 8))) return rc;
    if ((rc = upload(c, c->tmp[1], h_off, (size_t)(T + 1) * 8))) return rc;
    if ((rc = upload(c, c->tmp[2], es.data(), (size_t)n * 4))) return rc;
    HIPCHK(c, c->tmp[3].reserve((size_t)n * 8));
    hipLaunchKernelGGL(series_maxpool_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream,
                       c->tmp[0].as<double>(), c->tmp[3].as<double>(), c->tmp[1].as<int64_t>(),
                       c->tmp[2].as<int32_t>(), n, window, pad);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h_out, c->tmp[3].p, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, host_sync(c));
    return VDET_OK;
}

int vdet_series_interp_f64(vdet_ctx *c, const double *h_x, const double *h_y, const int64_t *h_koff,
                           const double *h_q, const int64_t *h_qoff, int64_t T, int K, double *h_out)
{
    if (!c || T < 0 || K < 1) return VDET_EINVAL;
    if (T == 0) return VDET_OK;
    if (!h_x || !h_y || !h_koff || !h_q || !h_qoff || !h_out) return fail(c, VDET_EINVAL, "null buffer");
    const int64_t nk = h_koff[T], nq = h_qoff[T];
    for (int64_t t = 0; t < T; ++t)
        if (h_koff[t + 1] - h_koff[t] < 2) return fail(c, VDET_EINVAL, "interpolation needs at least 2 knots");
    if (nq == 0) return VDET_OK;
    std::vector<int32_t> qs((size_t)nq);
    for (int64_t t = 0; t < T; ++t)
        for (int64_t e = h_qoff[t]; e < h_qoff[t + 1]; ++e) qs[(size_t)e] = (int32_t)t;
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    int rc;
    if ((rc = upload(c, c->tmp[0], h_x, (size_t)nk * 8))) return rc;
    if ((rc = upload(c, c->tmp[1], h_y, (size_t)nk * K * 8))) return rc;
    if ((rc = upload(c, c->tmp[2], h_koff, (size_t)(T + 1) * 8))) return rc;
    if ((rc = upload(c, c->tmp[3], h_q, (size_t)nq * 8))) return rc;
    if ((rc = upload(c, c->tmp[4], h_qoff, (size_t)(T + 1) * 8))) return rc;
    if ((rc = upload(c, c->tmp[5], qs.data(), (size_t)nq * 4))) return rc;
    HIPCHK(c, c->tmp[6].reserve((size_t)nq * K * 8));
    hipLaunchKernelGGL(series_interp_kernel, dim3((unsigned)((nq * K + 255) / 256)), dim3(256), 0, c->stream,
                       c->tmp[0].as<double>(), c->tmp[1].as<double>(), c->tmp[2].as<int64_t>(), c->tmp[3].as<double>(),
                       c->tmp[4].as<int64_t>(), c->tmp[5].as<int32_t>(), nq, K, c->tmp[6].as<double>());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h_out, c->tmp[6].p, (size_t)nq * K * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, host_sync(c));
    return VDET_OK;
}

int vdet_threshold_topk(vdet_ctx *c, const void *h_scores, int is_f64, int64_t B, int64_t ld, int col0, int ncls,
                        double thresh, int k, int32_t *h_idx, int32_t *h_cnt)
{
    if (!c || B < 0 || ncls < 0 || k < 0 || col0 < 0 || ld < col0 + ncls) return VDET_EINVAL;
    if (ncls == 0) return VDET_OK;
    if (!h_cnt || (k > 0 && !h_idx)) return fail(c, VDET_EINVAL, "null buffer");
    if (B == 0) { memset(h_cnt, 0, (size_t)ncls * 4); return VDET_OK; }
    if (!h_scores) return fail(c, VDET_EINVAL, "null buffer");
    const size_t es = is_f64 ? 8 : 4;
    const size_t lds = ((es * B + 15) & ~(size_t)15) + (((size_t)4 * B + 15) & ~(size_t)15) + 4 * 260;
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    if (!c->topk_attr_set) {
        HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void *>(threshold_topk_kernel<float>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->max_lds));
        HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void *>(threshold_topk_kernel<double>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->max_lds));
        c->topk_attr_set = true;
    }
    if (lds > c->max_lds) return fail(c, VDET_EINVAL, "too many boxes per frame for threshold_topk (%lld)", (long long)B);
    int rc;
    if ((rc = upload(c, c->tmp[0], h_scores, (size_t)B * ld * es))) return rc;
    HIPCHK(c, c->tmp[1].reserve((size_t)ncls * std::max(k, 1) * 4));
    HIPCHK(c, c->tmp[2].reserve((size_t)ncls * 4));
    if (is_f64)
        hipLaunchKernelGGL(threshold_topk_kernel<double>, dim3(ncls), dim3(256), lds, c->stream, c->tmp[0].as<double>(),
                           B, ld, col0, thresh, k, c->tmp[1].as<int32_t>(), c->tmp[2].as<int32_t>());
    else
        hipLaunchKernelGGL(threshold_topk_kernel<float>, dim3(ncls), dim3(256), lds, c->stream, c->tmp[0].as<float>(),
                           B, ld, col0, thresh, k, c->tmp[1].as<int32_t>(), c->tmp[2].as<int32_t>());
    HIPCHK(c, hipGetLastError());
    if (k > 0) HIPCHK(c, hipMemcpyAsync(h_idx, c->tmp[1].p, (size_t)ncls * k * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(h_cnt, c->tmp[2].p, (size_t)ncls * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, host_sync(c));
    return VDET_OK;
}

int vdet_conv1d_f32(vdet_ctx *c, const float *h_in, int Cin, int L, const float *h_w, const float *h_b, int Cout, int K,
                    int act, float *h_out)
{
    if (!c || Cin < 1 || Cout < 1 || L < 0 || K < 1 || K % 2 != 1 || act < 0 || act > 2)
        return c ? fail(c, VDET_EINVAL, "bad conv1d arguments") : VDET_EINVAL;
    if (L == 0) return VDET_OK;
    if (!h_in || !h_w || !h_b || !h_out) return fail(c, VDET_EINVAL, "null buffer");
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    int rc;
    if ((rc = upload(c, c->tmp[0], h_in, (size_t)Cin * L * 4))) return rc;
    if ((rc = upload(c, c->tmp[1], h_w, (size_t)Cout * Cin * K * 4))) return rc;
    if ((rc = upload(c, c->tmp[2], h_b, (size_t)Cout * 4))) return rc;
    HIPCHK(c, c->tmp[3].reserve((size_t)Cout * L * 4));
    HIPCHK(c, c->tmp[4].reserve((size_t)Cout * L * 4));
    const int n = Cout * L;
    hipLaunchKernelGGL(conv1d_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->tmp[0].as<float>(), Cin, L,
                       c->tmp[1].as<float>(), c->tmp[2].as<float>(), Cout, K, act == 1 ? 1 : 0, c->tmp[3].as<float>());
    float *res = c->tmp[3].as<float>();
    if (act == 2) {
        hipLaunchKernelGGL(softmax_channels_kernel, dim3((L + 255) / 256), dim3(256), 0, c->stream, c->tmp[3].as<float>(),
                           Cout, L, c->tmp[4].as<float>());
        res = c->tmp[4].as<float>();
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h_out, res, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, host_sync(c));
    return VDET_OK;
}

// ---------------------------------------------------------------------------------------------
static int temporal_launch(vdet_ctx *c, int mode, const float *d_in, float *d_out, int64_t F, int64_t S, int W,
                           float pad, float bias, const Taps &taps, const int2 *d_seg = nullptr)
{
    if (F == 0 || S == 0) return VDET_OK;
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    StageTimer tm(c, ST_TEMPORAL);
    const bool vec = (S % 4 == 0) && (((uintptr_t)d_in | (uintptr_t)d_out) & 15) == 0 && (W == 3 || W == 5 || W == 7 || W == 9);
    if (vec) {
        const int64_t S4 = S / 4;
        const unsigned gx = (unsigned)((S4 + 255) / 256);
        // few series (tubelet tracks): split the frame axis so the chip is still filled
        int64_t chunks = 1;
        if ((int64_t)gx < 4 * c->n_cu) chunks = std::min<int64_t>(std::max<int64_t>(F / 16, 1), (4 * c->n_cu + gx - 1) / gx);
        chunks = std::min<int64_t>(chunks, 65535);
        const int64_t fchunk = (F + chunks - 1) / chunks;
        const dim3 grid(gx, (unsigned)((F + fchunk - 1) / fchunk));
        const float4 *in4 = reinterpret_cast<const float4 *>(d_in);
        float4 *out4 = reinterpret_cast<float4 *>(d_out);
#define VDET_TL(WW, MM) hipLaunchKernelGGL((temporal_vec4_kernel<WW, MM>), grid, dim3(256), 0, c->stream, in4, out4, F, S4, fchunk, pad, bias, taps, d_seg)
        if (mode == 0) {
            if (W == 3) VDET_TL(3, 0); else if (W == 5) VDET_TL(5, 0); else if (W == 7) VDET_TL(7, 0); else VDET_TL(9, 0);
        } else {
            if (W == 3) VDET_TL(3, 1); else if (W == 5) VDET_TL(5, 1); else if (W == 7) VDET_TL(7, 1); else VDET_TL(9, 1);
        }
#undef VDET_TL
    } else {
        const int64_t n = F * S;
        const dim3 grid((unsigned)((n + 255) / 256));
        if (mode == 0) hipLaunchKernelGGL(temporal_scalar_kernel<0>, grid, dim3(256), 0, c->stream, d_in, d_out, F, S, W, pad, bias, taps, d_seg);
        else hipLaunchKernelGGL(temporal_scalar_kernel<1>, grid, dim3(256), 0, c->stream, d_in, d_out, F, S, W, pad, bias, taps, d_seg);
    }
    HIPCHK(c, hipGetLastError());
    return VDET_OK;
}

int vdet_temporal_maxpool_f32(vdet_ctx *c, const float *d_in, float *d_out, int64_t F, int64_t S, int window, float pad)
{
    if (!c) return VDET_EINVAL;
    if (window < 1 || window % 2 != 1) return fail(c, VDET_EINVAL, "Window size must be odd!");
    if (F < 0 || S < 0 || !fits_upto(1ll << 40, {F, S}) || (F * S > 0 && (!d_in || !d_out || d_in == d_out)))
        return fail(c, VDET_EINVAL, "bad temporal_maxpool arguments");
    Taps taps{};
    return temporal_launch(c, 0, d_in, d_out, F, S, window, pad, 0.0f, taps);
}

int vdet_temporal_conv_f32(vdet_ctx *c, const float *d_in, float *d_out, int64_t F, int64_t S, const float *h_taps,
                           int K, float bias, float pad)
{
    if (!c) return VDET_EINVAL;
    if (K < 1 || K % 2 != 1 || K > 31 || !h_taps) return fail(c, VDET_EINVAL, "taps: K must be odd and <= 31");
    if (F < 0 || S < 0 || !fits_upto(1ll << 40, {F, S}) || (F * S > 0 && (!d_in || !d_out || d_in == d_out)))
        return fail(c, VDET_EINVAL, "bad temporal_conv arguments");
    Taps taps{};
    for (int k = 0; k < K; ++k) taps.w[k] = h_taps[k];
    return temporal_launch(c, 1, d_in, d_out, F, S, K, pad, bias, taps);
}

static int temporal_maxpool_conv_impl(vdet_ctx *c, const float *d_in, float *d_out_max, float *d_out_conv, int64_t F, int64_t S,
                                      int window, float pad_max, const float *h_taps, float bias, float pad_conv, const int2 *d_seg);

int vdet_temporal_maxpool_conv_f32(vdet_ctx *c, const float *d_in, float *d_out_max, float *d_out_conv, int64_t F, int64_t S,
                                   int window, float pad_max, const float *h_taps, float bias, float pad_conv)
{
    return temporal_maxpool_conv_impl(c, d_in, d_out_max, d_out_conv, F, S, window, pad_max, h_taps, bias, pad_conv, nullptr);
}

static int temporal_maxpool_conv_impl(vdet_ctx *c, const float *d_in, float *d_out_max, float *d_out_conv, int64_t F, int64_t S,
                                      int window, float pad_max, const float *h_taps, float bias, float pad_conv, const int2 *d_seg)
{
    if (!c) return VDET_EINVAL;
    if (window < 1 || window % 2 != 1) return fail(c, VDET_EINVAL, "Window size must be odd!");
    if (window > 31 || !h_taps) return fail(c, VDET_EINVAL, "taps: K must be odd and <= 31");
    if (F < 0 || S < 0 || !fits_upto(1ll << 40, {F, S}) ||
        (F * S > 0 && (!d_in || !d_out_max || !d_out_conv || d_in == d_out_max || d_in == d_out_conv || d_out_max == d_out_conv)))
        return fail(c, VDET_EINVAL, "bad temporal_maxpool_conv arguments");
    if (F == 0 || S == 0) return VDET_OK;
    const bool vec = (S % 4 == 0) && (((uintptr_t)d_in | (uintptr_t)d_out_max | (uintptr_t)d_out_conv) & 15) == 0 &&
                     (window == 3 || window == 5 || window == 7);
    if (!vec) {   // shapes the fused kernel does not cover: the two passes
        Taps t0{};
        int rc = temporal_launch(c, 0, d_in, d_out_max, F, S, window, pad_max, 0.0f, t0, d_seg);
        if (rc) return rc;
        for (int k = 0; k < window; ++k) t0.w[k] = h_taps[k];
        return temporal_launch(c, 1, d_in, d_out_conv, F, S, window, pad_conv, bias, t0, d_seg);
    }
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    Taps taps{};
    for (int k = 0; k < window; ++k) taps.w[k] = h_taps[k];
    StageTimer tm(c, ST_TEMPORAL);
    const int64_t S4 = S / 4;
    const unsigned gx = (unsigned)((S4 + 255) / 256);
    int64_t chunks = 1;
    if ((int64_t)gx < 4 * c->n_cu) chunks = std::min<int64_t>(std::max<int64_t>(F / 16, 1), (4 * c->n_cu + gx - 1) / gx);
    chunks = std::min<int64_t>(chunks, 65535);
    const int64_t fchunk = (F + chunks - 1) / chunks;
    const dim3 grid(gx, (unsigned)((F + fchunk - 1) / fchunk));
    const float4 *in4 = reinterpret_cast<const float4 *>(d_in);
    float4 *om = reinterpret_cast<float4 *>(d_out_max), *oc = reinterpret_cast<float4 *>(d_out_conv);
#define VDET_TB(WW) hipLaunchKernelGGL((temporal_both_vec4_kernel<WW>), grid, dim3(256), 0, c->stream, in4, om, oc, F, S4, fchunk, pad_max, pad_conv, bias, taps, d_seg)
    if (window == 3) VDET_TB(3); else if (window == 5) VDET_TB(5); else VDET_TB(7);
#undef VDET_TB
    HIPCHK(c, hipGetLastError());
    return VDET_OK;
}

// ---------------------------------------------------------------------------------------------
static int volume_pass_impl(vdet_ctx *c, const float *d_scores, int64_t F, int64_t B, int64_t C, int window, float pad_max,
                            const float *h_taps, float bias, float pad_conv, float *d_out_max, float *d_out_conv,
                            int use_score_thresh, float score_thresh, const int2 *d_seg);

int vdet_volume_pass(vdet_ctx *c, const float *d_scores, int64_t F, int64_t B, int64_t C, int window, float pad_max,
                     const float *h_taps, float bias, float pad_conv, float *d_out_max, float *d_out_conv,
                     int use_score_thresh, float score_thresh)
{
    return volume_pass_impl(c, d_scores, F, B, C, window, pad_max, h_taps, bias, pad_conv, d_out_max, d_out_conv, use_score_thresh,
                            score_thresh, nullptr);
}

// frame offsets of V concatenated videos -> per-frame {first, one past last} table on the device (kept in the context)
static int upload_segments(vdet_ctx *c, const int64_t *h_frame_off, int64_t V, int64_t *Ftot)
{
    Videos vs;
    const int rc = read_videos(c, h_frame_off, V, 0, &vs, true);      // (a video without frames is fine here)
    if (rc) return rc;
    if (vs.F > 0x7FFFFFF0ll) return fail(c, VDET_EINVAL, "too many frames");
    *Ftot = vs.F;
    // O(F) to build: keyed by the O(V) offsets, so the same offsets again neither build nor upload it
    return stage_keyed(c, c->segtab, h_frame_off, (size_t)(V + 1) * 8, (size_t)vs.F * sizeof(int2), [&](char *dst) {
        int2 *seg = reinterpret_cast<int2 *>(dst);
        for (int64_t v = 0; v < V; ++v)
            for (int64_t f = h_frame_off[v]; f < h_frame_off[v + 1]; ++f) seg[f] = make_int2((int)h_frame_off[v], (int)h_frame_off[v + 1]);
    });
}

int vdet_volume_pass_batch(vdet_ctx *c, const float *d_scores, const int64_t *h_frame_off, int64_t V, int64_t B, int64_t C,
                           int window, float pad_max, const float *h_taps, float bias, float pad_conv, float *d_out_max,
                           float *d_out_conv, int use_score_thresh, float score_thresh)
{
    if (!c) return VDET_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    int64_t F = 0;
    const int rc = upload_segments(c, h_frame_off, V, &F);
    if (rc) return rc;
    return volume_pass_impl(c, d_scores, F, B, C, window, pad_max, h_taps, bias, pad_conv, d_out_max, d_out_conv, use_score_thresh,
                            score_thresh, c->segtab.dev.as<int2>());
}

static int volume_pass_impl(vdet_ctx *c, const float *d_scores, int64_t F, int64_t B, int64_t C, int window, float pad_max,
                            const float *h_taps, float bias, float pad_conv, float *d_out_max, float *d_out_conv,
                            int use_score_thresh, float score_thresh, const int2 *d_seg)
{
    if (!c) return VDET_EINVAL;
    if (window < 1 || window % 2 != 1) return fail(c, VDET_EINVAL, "Window size must be odd!");
    if (window > 31) return fail(c, VDET_EINVAL, "taps: K must be odd and <= 31");
    if (F < 0 || B < 0 || C < 0 || !fits_upto(1ll << 40, {F, B, C})) return fail(c, VDET_EINVAL, "bad shape");
    if (F == 0 || B == 0 || C == 0) return VDET_OK;
    const bool conv = h_taps != nullptr;
    if (!d_scores || !d_out_max || (conv && !d_out_conv) || d_scores == d_out_max || (conv && (d_scores == d_out_conv || d_out_max == d_out_conv)))
        return fail(c, VDET_EINVAL, "bad volume_pass arguments");
    if (B > 32767 || !fits_upto(0x7FFFFFF0ll, {F, C}) || !fits_upto(0x7FFFFFF0ll, {F, B})) return fail(c, VDET_EINVAL, "volume too large");
    c->keys_valid = false;
    c->vpass_last_items = 0;
    // tile: TB boxes (a power of two, >= 16 so that a key row segment is >= 64 B) x C classes in <= NT * ITEMS float4;
    // 4 items per thread (the window of every item lives in registers: more would cost occupancy), 256 or 512 threads
    const int64_t C4 = C / 4;
    // the lean form (temporal_kernels.hpp: volume_pass_lean_kernel): 2 items per thread, 512 threads, window 3
    int items = 0, TB = 0, NT = 0;
    const int form = c->vpass_form;
    if (C % 4 == 0 && (window == 3 || window == 5) &&
        (((uintptr_t)d_scores | (uintptr_t)d_out_max | (uintptr_t)(conv ? d_out_conv : d_out_max)) & 15) == 0) {
        if (window == 3 && form == VDET_VPASS_LEAN) {
            int tb = 64;
            while (tb >= 16 && (int64_t)tb * C4 > 512 * 2) tb >>= 1;
            if (tb >= 16) { items = 2; TB = tb; NT = 512; }
        }
        if (!items) {
            for (int nt : {256, 512}) {
                int tb = 64;
                while (tb >= 16 && (int64_t)tb * C4 > (int64_t)nt * 4) tb >>= 1;
                if (tb >= 16 && (nt == 512 || tb >= 32)) { items = 4; TB = tb; NT = nt; break; }
            }
        }
        if (items && (size_t)2 * C4 * TB * 16 > c->max_lds / 2) items = 0;
    }
    // one resident block per compute unit: the dynamic LDS is padded past half of a unit's (the kernel touches its tile only).
    // VDET_VPASS_AUTO takes it for an asynchronous context with the cache on (the multi-video pipeline, whose streams share the
    // chip): 4 videos in flight it measured 0.17-0.27 ms of 8.9-9.0 per step, the lean kernel nothing (LABNOTES "Lean volume pass")
    const bool one_per_cu = items == 4 && (form == VDET_VPASS_ONE_PER_CU ||
                                           (form == VDET_VPASS_AUTO && c->async_enabled && c->cache_enabled && window == 3 && NT == 512));
    if (!items) {
        // shapes the fused kernel does not cover: the temporal pass(es) now, the key transpose with the sort
        if (conv) return temporal_maxpool_conv_impl(c, d_scores, d_out_max, d_out_conv, F, B * C, window, pad_max, h_taps, bias, pad_conv, d_seg);
        Taps t0{};
        return temporal_launch(c, 0, d_scores, d_out_max, F, B * C, window, pad_max, 0.0f, t0, d_seg);
    }
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    // c->tkeys is rewritten (and possibly reallocated) below: sorted lists stay valid only if they are the lists of
    // exactly these keys (the tracking kernels read keys and lists together)
    if (!lists_match(c, ListsKey{d_scores, C, VDET_LAYOUT_FBC, use_score_thresh ? 1 : 0, score_thresh, 0}, F, B)) c->lists_valid = false;
    HIPCHK(c, c->tkeys.reserve((size_t)(F * C * B) * 4));
    Taps taps{};
    if (conv) for (int k = 0; k < window; ++k) taps.w[k] = h_taps[k];
    const int ntiles = (int)((B + TB - 1) / TB);
    int64_t chunks = std::min<int64_t>(std::max<int64_t>(F / 8, 1), (8 * c->n_cu + ntiles - 1) / ntiles);
    chunks = std::max<int64_t>(1, std::min<int64_t>(chunks, 65535));
    // frames per chunk: the formula's, or the forced one (vdet_set_vpass) raised until the chunks fit the grid's y dimension
    const int fchunk = c->vpass_fchunk > 0 ? (int)std::min<int64_t>(std::max<int64_t>(c->vpass_fchunk, (F + 65534) / 65535), F)
                                           : (int)((F + chunks - 1) / chunks);
    const int64_t nchunks = (F + fchunk - 1) / fchunk;
    // the lean kernel's blocks stride over the (tile, chunk) list, 2 of them per compute unit; the current kernel: a block per
    // (tile, chunk)
    const dim3 grid = items == 2 ? dim3((unsigned)std::min<int64_t>(nchunks * ntiles, 2 * (int64_t)c->n_cu))
                                 : dim3((unsigned)ntiles, (unsigned)nchunks);
    size_t lds = (size_t)2 * C4 * TB * 16;
    if (one_per_cu) lds = std::max(lds, c->max_lds / 2 + 16);
    int tb_shift = 0;
    while ((1 << tb_shift) < TB) ++tb_shift;
    const void *fn = nullptr;
#define VDET_VP(WW, CV, NTV) reinterpret_cast<const void *>(volume_pass_kernel<WW, 4, CV, NTV>)
#define VDET_VPL(CV) reinterpret_cast<const void *>(volume_pass_lean_kernel<3, 2, CV, 512>)
    if (items == 2) fn = conv ? VDET_VPL(true) : VDET_VPL(false);
    else if (window == 3) fn = NT == 256 ? (conv ? VDET_VP(3, true, 256) : VDET_VP(3, false, 256)) : (conv ? VDET_VP(3, true, 512) : VDET_VP(3, false, 512));
    else fn = NT == 256 ? (conv ? VDET_VP(5, true, 256) : VDET_VP(5, false, 256)) : (conv ? VDET_VP(5, true, 512) : VDET_VP(5, false, 512));
    if (!c->vpass_attr_set) {
        for (const void *f : {VDET_VP(3, true, 256), VDET_VP(3, false, 256), VDET_VP(3, true, 512), VDET_VP(3, false, 512),
                              VDET_VP(5, true, 256), VDET_VP(5, false, 256), VDET_VP(5, true, 512), VDET_VP(5, false, 512),
                              VDET_VPL(true), VDET_VPL(false)})
            HIPCHK(c, hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->max_lds));
        c->vpass_attr_set = true;
    }
#undef VDET_VPL
#undef VDET_VP
    const float4 *in4 = reinterpret_cast<const float4 *>(d_scores);
    float4 *om = reinterpret_cast<float4 *>(d_out_max), *oc = reinterpret_cast<float4 *>(d_out_conv);
    uint32_t *keys = c->tkeys.as<uint32_t>();
    int Fi = (int)F, Bi = (int)B, C4i = (int)C4;
    void *args[] = {&in4, &om, &oc, &keys, &Fi, &Bi, &C4i, &TB, &tb_shift, (void *)&fchunk, &pad_max, &pad_conv, &bias, &taps,
                    &use_score_thresh, &score_thresh, (void *)&d_seg};
    {
        StageTimer tm(c, ST_TEMPORAL);
        HIPCHK(c, hipLaunchKernel(fn, grid, dim3((unsigned)NT), args, lds, c->stream));
    }
    HIPCHK(c, hipGetLastError());
    c->keysrc.scores = d_scores; c->keysrc.F = F; c->keysrc.B = B; c->keysrc.C = C;
    c->keysrc.use_thr = use_score_thresh ? 1 : 0; c->keysrc.thr = score_thresh;
    c->keys_valid = true;
    c->vpass_last_items = items + (one_per_cu ? 100 : 0);
    return VDET_OK;
}

// ---------------------------------------------------------------------------------------------
extern "C++" {
template <typename T>
static int svm_scores_impl(vdet_ctx *c, const T *h_feat, int64_t n, int64_t k, const T *h_W, const T *h_B, int64_t m, T *h_out)
{
    if (!c || n < 0 || k < 0 || m < 0) return VDET_EINVAL;
    if (n == 0 || m == 0) return VDET_OK;
    if ((k > 0 && (!h_feat || !h_W)) || !h_out) return fail(c, VDET_EINVAL, "null buffer");
    if (n * k > ((int64_t)1 << 34) || k * m > ((int64_t)1 << 34) || n * m > ((int64_t)1 << 34)) return fail(c, VDET_EINVAL, "matrix too large");
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    int rc;
    if ((rc = upload(c, c->tmp[0], h_feat, (size_t)(n * k) * sizeof(T)))) return rc;
    if ((rc = upload(c, c->tmp[1], h_W, (size_t)(k * m) * sizeof(T)))) return rc;
    if (h_B && (rc = upload(c, c->tmp[2], h_B, (size_t)m * sizeof(T)))) return rc;
    HIPCHK(c, c->tmp[3].reserve((size_t)(n * m) * sizeof(T)));
    {
        StageTimer tm(c, ST_OTHER);
        hipLaunchKernelGGL(svm_scores_kernel<T>, dim3((unsigned)((m + 63) / 64), (unsigned)((n + 63) / 64)), dim3(256), 0, c->stream,
                           c->tmp[0].as<T>(), c->tmp[1].as<T>(), h_B ? c->tmp[2].as<T>() : (const T *)nullptr, n, k, m, c->tmp[3].as<T>());
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h_out, c->tmp[3].p, (size_t)(n * m) * sizeof(T), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, host_sync(c));
    return VDET_OK;
}
}  // extern "C++"

int vdet_svm_scores_f64(vdet_ctx *c, const double *h_feat, int64_t n, int64_t k, const double *h_W, const double *h_B, int64_t m,
                        double *h_out)
{
    return svm_scores_impl<double>(c, h_feat, n, k, h_W, h_B, m, h_out);
}

int vdet_svm_scores_f32(vdet_ctx *c, const float *h_feat, int64_t n, int64_t k, const float *h_W, const float *h_B, int64_t m,
                        float *h_out)
{
    return svm_scores_impl<float>(c, h_feat, n, k, h_W, h_B, m, h_out);
}

// ---------------------------------------------------------------------------------------------
// Device evaluator (eval_kernels.hpp; the specification is vdetlib_amd/eval.py)
// ---------------------------------------------------------------------------------------------
int vdet_eval_gt_upload(vdet_ctx *c, const int32_t *h_vid, const int64_t *h_frame, const int32_t *h_slot, const double *h_boxes,
                        int64_t G, const int64_t *h_vid_nf, int64_t NV, int K, double *d_gt_boxes, int32_t *d_gt_off,
                        int64_t *d_vid_meta)
{
    if (!c) return VDET_EINVAL;
    if (G < 0 || NV < 0 || K < 1 || K > 65536) return fail(c, VDET_EINVAL, "bad ground-truth table shape");
    if ((G && (!h_vid || !h_frame || !h_slot || !h_boxes)) || (NV && !h_vid_nf) || !d_gt_off || (NV && !d_vid_meta))
        return fail(c, VDET_EINVAL, "null buffer");
    std::vector<int64_t> meta((size_t)NV * 2);
    int64_t total = 0;
    for (int64_t v = 0; v < NV; ++v) {
        if (h_vid_nf[v] < 0) return fail(c, VDET_EINVAL, "negative frame count");
        meta[2 * v] = total;
        meta[2 * v + 1] = h_vid_nf[v];
        if (!fits_upto(0x7FFFFFF0ll - total, {h_vid_nf[v], K})) return fail(c, VDET_EINVAL, "ground-truth table too large (videos x frames x classes >= 2^31)");
        total += h_vid_nf[v] * K;
    }
    auto cell = [&](int64_t i) -> int64_t {
        const int32_t v = h_vid[i], s = h_slot[i];
        if (v < 0 || v >= NV || s < 0 || s >= K || h_frame[i] < 0 || h_frame[i] >= meta[2 * v + 1]) return -1;
        return meta[2 * v] + h_frame[i] * K + s;
    };
    std::vector<int32_t> off((size_t)total + 1, 0);
    int64_t placed = 0;
    for (int64_t i = 0; i < G; ++i) {
        const int64_t o = cell(i);
        if (o < 0) continue;
        if (++off[(size_t)o + 1] > kEvalMaxGt)
            return fail(c, VDET_EINVAL, "more than %d ground-truth boxes in one (video, frame, class)", kEvalMaxGt);
        ++placed;
    }
    if (placed > 0x7FFFFFF0ll) return fail(c, VDET_EINVAL, "too many ground-truth boxes");
    for (int64_t o = 0; o < total; ++o) off[(size_t)o + 1] += off[(size_t)o];
    std::vector<int32_t> cur(off.begin(), off.end() - 1);
    std::vector<double> boxes((size_t)placed * 4);
    for (int64_t i = 0; i < G; ++i) {           // annotation order within every cell
        const int64_t o = cell(i);
        if (o < 0) continue;
        const int32_t p = cur[(size_t)o]++;
        for (int q = 0; q < 4; ++q) boxes[(size_t)p * 4 + q] = h_boxes[i * 4 + q];
    }
    HIPCHK(c, hipSetDevice(c->device));
    if (placed) HIPCHK(c, hipMemcpyAsync(d_gt_boxes, boxes.data(), boxes.size() * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_gt_off, off.data(), off.size() * 4, hipMemcpyHostToDevice, c->stream));
    if (NV) HIPCHK(c, hipMemcpyAsync(d_vid_meta, meta.data(), meta.size() * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, host_sync(c));        // the host vectors die here
    return VDET_OK;
}

static int eval_gt_args(vdet_ctx *c, const double *d_gt_boxes, const int32_t *d_gt_off, const int64_t *d_vid_meta, int K, int rule,
                 double iou_thr, EvGt &g)
{
    if (!d_gt_off || !d_vid_meta || K < 1 || K > 65536) return fail(c, VDET_EINVAL, "bad ground-truth CSR");
    if (rule != 0 && rule != 1) return fail(c, VDET_EINVAL, "rule must be 0 (VOC) or 1 (ILSVRC)");
    g = EvGt{d_gt_boxes, d_gt_off, d_vid_meta, K, rule, iou_thr};
    return VDET_OK;
}

// the dense results of a match launch (c->ev_dtp / ev_dsc / ev_dslot, N entries) -> appended to the stream at st_len, in
// order; one host wait to learn the count
static int eval_compact(vdet_ctx *c, int64_t N, int32_t *st_slot, double *st_sc, uint8_t *st_tp, int64_t st_len, int64_t *h_count)
{
    const int64_t nb = (N + kEvalTile - 1) / kEvalTile;
    HIPCHK(c, c->ev_bcnt.reserve((size_t)nb * 8 + 8));
    HIPCHK(c, c->ev_boff.reserve((size_t)nb * 8 + 8));
    int64_t *total = c->ev_bcnt.as<int64_t>() + nb;
    {
        StageTimer tm(c, ST_OTHER);
        hipLaunchKernelGGL(eval_count_kernel, dim3((unsigned)nb), dim3(256), 0, c->stream, c->ev_dtp.as<int8_t>(), N,
                           c->ev_bcnt.as<int64_t>());
        hipLaunchKernelGGL(eval_scan_kernel<int64_t>, dim3(1), dim3(1024), 0, c->stream, c->ev_bcnt.as<int64_t>(), nb,
                           c->ev_boff.as<int64_t>(), total);
        hipLaunchKernelGGL(eval_scatter_kernel, dim3((unsigned)nb), dim3(256), 0, c->stream, c->ev_dtp.as<int8_t>(),
                           c->ev_dsc.as<double>(), c->ev_dslot.as<int32_t>(), N, c->ev_boff.as<int64_t>(), st_len, st_slot, st_sc, st_tp);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h_count, total, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, host_sync(c));
    return VDET_OK;
}

static int eval_dense(vdet_ctx *c, int64_t N)
{
    HIPCHK(c, c->ev_dtp.reserve((size_t)N));
    HIPCHK(c, c->ev_dsc.reserve((size_t)N * 8));
    HIPCHK(c, c->ev_dslot.reserve((size_t)N * 4));
    return VDET_OK;
}

int vdet_eval_match_tracks_batch(vdet_ctx *c, const double *d_gt_boxes, const int32_t *d_gt_off, const int64_t *d_vid_meta, int K,
                                 int rule, double iou_thr, const int32_t *h_vid, const int64_t *h_frame_off, int64_t V, int64_t C,
                                 int T, const float *d_boxes, int box_stride, const void *d_scores, int scores_f64,
                                 const int32_t *d_ntracks, const int32_t *h_col_slot, int32_t *d_st_slot, double *d_st_score,
                                 uint8_t *d_st_tp, int64_t st_len, int64_t st_cap, int64_t *h_count)
{
    if (!c) return VDET_EINVAL;
    EvGt g;
    int rc = eval_gt_args(c, d_gt_boxes, d_gt_off, d_vid_meta, K, rule, iou_thr, g);
    if (rc) return rc;
    if (!h_count || !h_vid || !h_frame_off || !h_col_slot) return fail(c, VDET_EINVAL, "null buffer");
    *h_count = 0;
    if (V < 1 || C < 1 || C > 65535 || T < 0 || T > kEvalMaxT || (box_stride != 4 && box_stride != 5))
        return fail(c, VDET_EINVAL, "bad shape (1 <= C <= 65535, 0 <= T <= %d, box stride 4 or 5)", kEvalMaxT);
    Videos vs;
    if ((rc = read_videos(c, h_frame_off, V, 0, &vs))) return rc;
    const int64_t Ft = vs.F;
    if (Ft > 0x7FFFFFF0ll || !fits_upto(0x7FFFFFF0ll, {C, T, Ft})) return fail(c, VDET_EINVAL, "too many tubelet boxes");
    const int64_t N = C * T * Ft;
    if (T == 0) return VDET_OK;
    if (!d_boxes || !d_scores || !d_ntracks || !d_st_slot || !d_st_score || !d_st_tp) return fail(c, VDET_EINVAL, "null buffer");
    if (st_len < 0 || st_len + N > st_cap) return fail(c, VDET_EINVAL, "stream capacity too small (%lld + %lld > %lld)",
                                                      (long long)st_len, (long long)N, (long long)st_cap);
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    // host tables: column slots [C] i32 | video table indices [V] i32 | frame offsets [V+1] i64
    const size_t o_vid = ((size_t)C * 4 + 7) & ~(size_t)7, o_off = (o_vid + (size_t)V * 4 + 7) & ~(size_t)7;
    std::vector<char> tab(o_off + (size_t)(V + 1) * 8);
    memcpy(tab.data(), h_col_slot, (size_t)C * 4);
    memcpy(tab.data() + o_vid, h_vid, (size_t)V * 4);
    memcpy(tab.data() + o_off, h_frame_off, (size_t)(V + 1) * 8);
    if ((rc = eval_dense(c, N))) return rc;
    HIPCHK(c, c->ev_tab.reserve(tab.size()));
    HIPCHK(c, hipMemcpyAsync(c->ev_tab.p, tab.data(), tab.size(), hipMemcpyHostToDevice, c->stream));
    char *tb = c->ev_tab.as<char>();
    {
        StageTimer tm(c, ST_OTHER);
        hipLaunchKernelGGL(eval_match_tracks_kernel, dim3((unsigned)Ft, (unsigned)C), dim3(64), 0, c->stream, g,
                           reinterpret_cast<const int64_t *>(tb + o_off), (int)V, reinterpret_cast<const int32_t *>(tb + o_vid), (int)C,
                           T, d_boxes, box_stride, scores_f64 ? static_cast<const double *>(d_scores) : (const double *)nullptr,
                           scores_f64 ? (const float *)nullptr : static_cast<const float *>(d_scores), d_ntracks,
                           reinterpret_cast<const int32_t *>(tb), c->ev_dtp.as<int8_t>(), c->ev_dsc.as<double>(),
                           c->ev_dslot.as<int32_t>());
    }
    HIPCHK(c, hipGetLastError());
    return eval_compact(c, N, d_st_slot, d_st_score, d_st_tp, st_len, h_count);   // (its host wait also retires `tab`)
}

int vdet_eval_match_tracks(vdet_ctx *c, const double *d_gt_boxes, const int32_t *d_gt_off, const int64_t *d_vid_meta, int K, int rule,
                           double iou_thr, int vid, int64_t F, int64_t C, int T, const float *d_boxes, int box_stride,
                           const void *d_scores, int scores_f64, const int32_t *d_ntracks, const int32_t *h_col_slot,
                           int32_t *d_st_slot, double *d_st_score, uint8_t *d_st_tp, int64_t st_len, int64_t st_cap,
                           int64_t *h_count)
{
    const int64_t foff[2] = {0, F};
    return vdet_eval_match_tracks_batch(c, d_gt_boxes, d_gt_off, d_vid_meta, K, rule, iou_thr, &vid, foff, 1, C, T, d_boxes,
                                        box_stride, d_scores, scores_f64, d_ntracks, h_col_slot, d_st_slot, d_st_score, d_st_tp,
                                        st_len, st_cap, h_count);
}

int vdet_eval_match_keep(vdet_ctx *c, const double *d_gt_boxes, const int32_t *d_gt_off, const int64_t *d_vid_meta, int K, int rule,
                         double iou_thr, int vid, const float *d_boxes, const float *d_scores, int layout, int64_t F, int64_t B,
                         int64_t C, const int32_t *d_keep_idx, const int32_t *d_keep_cnt, int64_t cap, const int32_t *h_col_slot,
                         int32_t *d_st_slot, double *d_st_score, uint8_t *d_st_tp, int64_t st_len, int64_t st_cap,
                         int64_t *h_count)
{
    if (!c) return VDET_EINVAL;
    EvGt g;
    int rc = eval_gt_args(c, d_gt_boxes, d_gt_off, d_vid_meta, K, rule, iou_thr, g);
    if (rc) return rc;
    if (!h_count || !h_col_slot) return fail(c, VDET_EINVAL, "null buffer");
    *h_count = 0;
    if (layout != VDET_LAYOUT_FBC && layout != VDET_LAYOUT_FCB) return fail(c, VDET_EINVAL, "bad layout");
    if (F < 1 || B < 1 || C < 1 || C > 65535 || cap < 0 || B > 0x7FFFFFFF) return fail(c, VDET_EINVAL, "bad shape");
    if (F > 0x7FFFFFF0ll || !fits_upto(0x7FFFFFF0ll, {F, C, cap}) || !fits_upto(1ll << 40, {F, B, C})) return fail(c, VDET_EINVAL, "too many kept entries");
    const int64_t N = F * C * cap;
    if (cap == 0) return VDET_OK;
    if (!d_boxes || !d_scores || !d_keep_idx || !d_keep_cnt || !d_st_slot || !d_st_score || !d_st_tp)
        return fail(c, VDET_EINVAL, "null buffer");
    if (st_len < 0 || st_len + N > st_cap) return fail(c, VDET_EINVAL, "stream capacity too small (%lld + %lld > %lld)",
                                                      (long long)st_len, (long long)N, (long long)st_cap);
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    if ((rc = eval_dense(c, N))) return rc;
    if ((rc = upload(c, c->ev_tab, h_col_slot, (size_t)C * 4))) return rc;
    {
        StageTimer tm(c, ST_OTHER);
        hipLaunchKernelGGL(eval_match_keep_kernel, dim3((unsigned)F, (unsigned)C), dim3(64), 0, c->stream, g, vid, (int)C, (int)B,
                           layout, d_boxes, d_scores, d_keep_idx, d_keep_cnt, cap, c->ev_tab.as<int32_t>(), c->ev_dtp.as<int8_t>(),
                           c->ev_dsc.as<double>(), c->ev_dslot.as<int32_t>(), &c->d_cnt->status);
    }
    HIPCHK(c, hipGetLastError());
    return eval_compact(c, N, d_st_slot, d_st_score, d_st_tp, st_len, h_count);
}

int vdet_eval_ap(vdet_ctx *c, const int32_t *d_st_slot, const double *d_st_score, const uint8_t *d_st_tp, int64_t n, int K,
                 const int64_t *d_ngt, double *d_ap, int32_t *d_perm)
{
    if (!c) return VDET_EINVAL;
    if (n < 0 || n > 0x7FFFFFF0ll || K < 1 || K > 65536) return fail(c, VDET_EINVAL, "bad shape (stream < 2^31, 1 <= K <= 65536)");
    if (!d_ngt || !d_ap || (n && (!d_st_slot || !d_st_score || !d_st_tp))) return fail(c, VDET_EINVAL, "null buffer");
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    const uint64_t *val = nullptr;
    if (n) {
        const int64_t nb = (n + kEvalTile - 1) / kEvalTile;
        for (int i = 0; i < 2; ++i) {
            HIPCHK(c, c->ev_key[i].reserve((size_t)n * 8));
            HIPCHK(c, c->ev_val[i].reserve((size_t)n * 8));
        }
        HIPCHK(c, c->ev_hist.reserve((size_t)nb * 256 * 8));
        uint32_t *hist = c->ev_hist.as<uint32_t>(), *hoff = hist + nb * 256;
        const int passes = 8 + (K <= 1 ? 0 : (K <= 256 ? 1 : 2));
        StageTimer tm(c, ST_SORT);
        hipLaunchKernelGGL(eval_key_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, d_st_slot, d_st_score, n,
                           c->ev_key[0].as<uint64_t>(), c->ev_val[0].as<uint64_t>());
        int cur = 0;
        for (int p = 0; p < passes; ++p) {
            hipLaunchKernelGGL(eval_hist_kernel, dim3((unsigned)nb), dim3(256), 0, c->stream, c->ev_key[cur].as<uint64_t>(),
                               c->ev_val[cur].as<uint64_t>(), n, p, hist);
            hipLaunchKernelGGL(eval_scan_kernel<uint32_t>, dim3(1), dim3(1024), 0, c->stream, hist, nb * 256, hoff, (uint32_t *)nullptr);
            hipLaunchKernelGGL(eval_radix_scatter_kernel, dim3((unsigned)nb), dim3(256), 0, c->stream, c->ev_key[cur].as<uint64_t>(),
                               c->ev_val[cur].as<uint64_t>(), n, p, hoff, c->ev_key[cur ^ 1].as<uint64_t>(),
                               c->ev_val[cur ^ 1].as<uint64_t>());
            cur ^= 1;
        }
        val = c->ev_val[cur].as<uint64_t>();
        if (d_perm)
            hipLaunchKernelGGL(eval_perm_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, val, n, d_perm);
    }
    {
        StageTimer tm(c, ST_OTHER);
        hipLaunchKernelGGL(eval_ap_kernel, dim3((unsigned)K), dim3(256), 0, c->stream, val, d_st_tp, n, d_ngt, d_ap);
    }
    HIPCHK(c, hipGetLastError());
    return VDET_OK;
}

// ---------------------------------------------------------------------------------------------
// Device TCN (tcn_kernels.hpp)
// ---------------------------------------------------------------------------------------------
// h_layers [n_layers][3] = (Cout, Cin, K); h_params = W0 | b0 | W1 | b1 | ... (W [Cout, Cin, K] row-major).  The parameters
// are uploaded when their bytes differ from the resident ones (vdet_query(ctx, 10) counts the uploads).
static int tcn_net_args(vdet_ctx *c, const float *h_params, const int32_t *h_layers, int n_layers, int cin, TcnNet &net)
{
    if (!h_params || !h_layers) return fail(c, VDET_EINVAL, "null buffer");
    if (n_layers < 1 || n_layers > kTcnMaxLayers) return fail(c, VDET_EINVAL, "a net has 1 to %d layers", kTcnMaxLayers);
    if (cin < 1 || cin > kTcnMaxChannels) return fail(c, VDET_EINVAL, "a net has 1 to %d input channels", kTcnMaxChannels);
    net = TcnNet{};
    net.n = n_layers; net.cin = cin; net.maxc = cin; net.halo = 0;
    int64_t off = 0;
    int prev = cin;
    for (int i = 0; i < n_layers; ++i) {
        const int co = h_layers[3 * i], ci = h_layers[3 * i + 1], k = h_layers[3 * i + 2];
        if (co < 1 || co > kTcnMaxChannels) return fail(c, VDET_EINVAL, "layer %d: 1 to %d channels", i, kTcnMaxChannels);
        if (ci != prev) return fail(c, VDET_EINVAL, "layer shapes do not chain: layer %d takes %d channels after %d", i, ci, prev);
        if (k < 1 || k % 2 != 1 || k > kTcnMaxK) return fail(c, VDET_EINVAL, "layer %d: the kernel size must be odd and <= %d", i, kTcnMaxK);
        net.l[i].cin = ci; net.l[i].cout = co; net.l[i].k = k;
        net.l[i].woff = (int)off; off += (int64_t)co * ci * k;
        net.l[i].boff = (int)off; off += co;
        if (off > 0x7FFFFFF0ll / 4) return fail(c, VDET_EINVAL, "net too large");
        net.maxc = std::max(net.maxc, co);
        net.halo += k / 2;
        prev = co;
    }
    if (prev != 2) return fail(c, VDET_EINVAL, "the last layer must produce 2 channels (probs[:, 1, :] is the score)");
    int rem = 0;
    for (int i = n_layers - 1; i >= 0; --i) { net.l[i].rem = rem; rem += net.l[i].k / 2; }
    return stage_table(c, c->tcn_params, h_params, (size_t)off * 4);
}

// The network launch over ntub tubelet descriptors; Lmax bounds every series length.  Path by size (DESIGN.md "Device TCN"):
// whole series in LDS; else tiles of the largest width the LDS budget holds; else (net too wide for a useful tile) the
// global-memory activations, tiled so that the scratch stays within 256 MiB.
static int tcn_launch_net(vdet_ctx *c, const TcnNet &net, const float *d_x, const int32_t *d_frames, const int64_t *d_base,
                          const int32_t *d_len, int64_t ntub, int64_t Lmax, float *d_out)
{
    if (ntub <= 0) return VDET_OK;
    const int lmax = (int)std::max<int64_t>(std::min<int64_t>(Lmax, 0x3FFFFFF0), 1);
    const int min_tile = std::max(kTcnMinTile, 2 * net.halo);
    const int64_t per_pos = (int64_t)8 * net.maxc;            // two buffers x maxc floats per staged position
    const int64_t fit = kTcnLdsBudget / per_pos - 2 * net.halo;   // widest tile the LDS budget holds
    const float *params = c->tcn_params.dev.as<float>();
    StageTimer tm(c, ST_OTHER);
    if (!c->tcn_global && fit >= std::min(lmax, min_tile)) {
        int tile = (int)std::min<int64_t>(fit, lmax);
        if (c->tcn_tiled) tile = std::min(tile, min_tile);
        const size_t lds = (size_t)per_pos * (tile + 2 * net.halo);
        const unsigned grid = (unsigned)std::min<int64_t>(ntub, (int64_t)64 * c->n_cu);
        hipLaunchKernelGGL(tcn_net_kernel<false>, dim3(grid), dim3(kTcnThreads), lds, c->stream, net, params, d_x, d_frames, d_base,
                           d_len, ntub, tile, (float *)nullptr, d_out);
    } else {
        int tile = std::min(lmax, std::max(256, min_tile));
        if (c->tcn_tiled) tile = std::min(tile, min_tile);
        const size_t per_wg = (size_t)per_pos * (tile + 2 * net.halo);
        const int64_t grid = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(ntub, (int64_t)2 * c->n_cu), ((int64_t)256 << 20) / (int64_t)per_wg));
        HIPCHK(c, c->tcn_scratch.reserve(per_wg * (size_t)grid));
        hipLaunchKernelGGL(tcn_net_kernel<true>, dim3((unsigned)grid), dim3(kTcnThreads), 0, c->stream, net, params, d_x, d_frames,
                           d_base, d_len, ntub, tile, c->tcn_scratch.as<float>(), d_out);
    }
    HIPCHK(c, hipGetLastError());
    return VDET_OK;
}

// The wide first layer (tcn_wide_layer_kernel) over the assembled tubelets: h0 = layer 0 of `net` on the segment table.
static void tcn_launch_wide(vdet_ctx *c, dim3 grid, const TcnLayer &l0, int relu, int nseg, int nx, int64_t ntub)
{
    const TcnSeg *segs = c->tcn_segs.dev.as<TcnSeg>();
    const float *params = c->tcn_params.dev.as<float>();
#define VDET_TCN_WIDE(A, KT)                                                                                                       \
    hipLaunchKernelGGL((tcn_wide_layer_kernel<A, KT>), grid, dim3(kTcnThreads), 0, c->stream, segs, nseg, l0.cin, l0.cout, l0.k, relu,  \
                       params + l0.woff, params + l0.boff, c->tcn_x.as<float>(), nx, c->tcn_frames.as<int32_t>(),                 \
                       c->tcn_base.as<int64_t>(), c->tcn_len.as<int32_t>(), ntub, c->tcn_h0.as<float>())
    // accumulator blocking by width (8 channels per wave; 2 for layers of at most 8), taps unrolled for K = 3 and 5
    if (l0.cout <= 8) {
        if (l0.k == 3) VDET_TCN_WIDE(2, 3);
        else if (l0.k == 5) VDET_TCN_WIDE(2, 5);
        else VDET_TCN_WIDE(2, 0);
    } else {
        if (l0.k == 3) VDET_TCN_WIDE(8, 3);
        else if (l0.k == 5) VDET_TCN_WIDE(8, 5);
        else VDET_TCN_WIDE(8, 0);
    }
#undef VDET_TCN_WIDE
}

// THE device TCN over tracks.  segs == nullptr: the narrow call, every input an assembled channel and the whole net in
// tcn_net_kernel.  Otherwise layer 0 reads the nseg segments (TcnSeg.c0 / xq filled here) and tcn_net_kernel runs the rest.
static int tcn_tracks_impl(vdet_ctx *c, const float *h_params, const int32_t *h_layers, int n_layers, const TcnChannels &ch,
                           TcnSeg *segs, int nseg, int cin, const int64_t *h_frame_off, int64_t V, int64_t C, int T,
                           const float *d_tracks, const int32_t *d_ntracks, const float *d_anchors, const void *d_det_score,
                           int det_f64, const double *d_gt_overlap, float *d_conv_score)
{
    Videos vs;
    int rc = read_videos(c, h_frame_off, V, 65535, &vs);
    if (rc) return rc;
    const int64_t Ft = vs.F, Fmax = vs.Fmax;
    if (C < 1 || T < 0 || !fits_upto(0x7FFFFFF0ll, {C, std::max(T, 1)})) return fail(c, VDET_EINVAL, "bad shape");
    bool need_gt = false, need_det = false;
    for (int q = 0; q < ch.n; ++q) {
        need_gt = need_gt || ch.code[q] == kChGtOverlap || ch.code[q] == kChLabel;
        need_det = need_det || ch.code[q] == kChDet;
    }
    if (need_gt && !d_gt_overlap) return fail(c, VDET_EINVAL, "the net reads gt_overlaps / labels: a gt_overlap buffer is needed");
    if (!fits_upto(0x7FFFFFF0ll, {C, T, Ft}) || !fits_upto(1ll << 40, {C, T, Ft, std::max(ch.n, 1)})) return fail(c, VDET_EINVAL, "too many tubelet boxes");
    const int64_t N = C * T * Ft;
    if (T == 0) return VDET_OK;
    if (!d_tracks || !d_ntracks || !d_anchors || (need_det && !d_det_score) || !d_conv_score) return fail(c, VDET_EINVAL, "null buffer");
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    TcnNet net;
    if ((rc = tcn_net_args(c, h_params, h_layers, n_layers, cin, net))) return rc;
    if (segs) {
        if (!fits_upto(1ll << 40, {N, net.l[0].cout})) return fail(c, VDET_EINVAL, "too many tubelet boxes");
        if ((rc = stage_table(c, c->tcn_segs, segs, (size_t)nseg * sizeof(TcnSeg)))) return rc;
    }
    const int64_t *d_foff = nullptr;
    if (V > 1) {
        if ((rc = stage_table(c, c->tcn_foff, h_frame_off, (size_t)(V + 1) * 8))) return rc;
        d_foff = c->tcn_foff.dev.as<int64_t>();
    }
    const int64_t ntub = V * C * T;
    HIPCHK(c, c->tcn_x.reserve((size_t)N * ch.n * 4));
    HIPCHK(c, c->tcn_frames.reserve((size_t)N * 4));
    HIPCHK(c, c->tcn_base.reserve((size_t)ntub * 8));
    HIPCHK(c, c->tcn_len.reserve((size_t)ntub * 4));
    if (segs) HIPCHK(c, c->tcn_h0.reserve((size_t)N * net.l[0].cout * 4));
    {
        StageTimer tm(c, ST_OTHER);
        hipLaunchKernelGGL(tcn_assemble_kernel, dim3((unsigned)(C * T), (unsigned)V), dim3(64), 0, c->stream, d_tracks, d_ntracks, d_anchors,
                           det_f64 ? static_cast<const double *>(d_det_score) : (const double *)nullptr,
                           det_f64 ? (const float *)nullptr : static_cast<const float *>(d_det_score), d_gt_overlap, d_foff, Ft, (int)C, T,
                           ch, c->tcn_x.as<float>(), c->tcn_frames.as<int32_t>(), c->tcn_base.as<int64_t>(), c->tcn_len.as<int32_t>(),
                           d_conv_score);
    }
    HIPCHK(c, hipGetLastError());
    if (!segs)
        return tcn_launch_net(c, net, c->tcn_x.as<float>(), c->tcn_frames.as<int32_t>(), c->tcn_base.as<int64_t>(), c->tcn_len.as<int32_t>(),
                              ntub, Fmax, d_conv_score);
    {
        StageTimer tm(c, ST_OTHER);
        const TcnLayer &l0 = net.l[0];
        const int64_t tiles = (Fmax + kTcnWideTile - 1) / kTcnWideTile;
        const dim3 grid((unsigned)std::min<int64_t>(ntub, (int64_t)64 * c->n_cu), (unsigned)std::min<int64_t>(tiles, 1024));
        const int relu = n_layers > 1;
        tcn_launch_wide(c, grid, l0, relu, nseg, ch.n, ntub);
    }
    HIPCHK(c, hipGetLastError());
    // layers 1 .. n-1 on h0 [cout0, L]; a one-layer net leaves the softmax alone (a net of zero layers)
    TcnNet tail{};
    tail.n = net.n - 1;
    tail.cin = tail.maxc = net.l[0].cout;
    for (int i = 0; i < tail.n; ++i) {
        tail.l[i] = net.l[i + 1];
        tail.maxc = std::max(tail.maxc, tail.l[i].cout);
        tail.halo += tail.l[i].k / 2;
    }
    return tcn_launch_net(c, tail, c->tcn_h0.as<float>(), c->tcn_frames.as<int32_t>(), c->tcn_base.as<int64_t>(), c->tcn_len.as<int32_t>(),
                          ntub, Fmax, d_conv_score);
}

int vdet_tcn_tracks_batch(vdet_ctx *c, const float *h_params, const int32_t *h_layers, int n_layers, const int32_t *h_channels,
                          int n_channels, const int64_t *h_frame_off, int64_t V, int64_t C, int T, const float *d_tracks,
                          const int32_t *d_ntracks, const float *d_anchors, const void *d_det_score, int det_f64,
                          const double *d_gt_overlap, float *d_conv_score)
{
    if (!c) return VDET_EINVAL;
    if (!h_channels || n_channels < 1 || n_channels > 16) return fail(c, VDET_EINVAL, "1 to 16 input channels");
    TcnChannels ch{};
    ch.n = n_channels;
    for (int q = 0; q < n_channels; ++q) {
        if (h_channels[q] < 0 || h_channels[q] >= kChCount) return fail(c, VDET_EINVAL, "unknown input channel code %d", h_channels[q]);
        ch.code[q] = h_channels[q];
    }
    return tcn_tracks_impl(c, h_params, h_layers, n_layers, ch, nullptr, 0, n_channels, h_frame_off, V, C, T, d_tracks, d_ntracks,
                           d_anchors, d_det_score, det_f64, d_gt_overlap, d_conv_score);
}

int vdet_tcn_tracks(vdet_ctx *c, const float *h_params, const int32_t *h_layers, int n_layers, const int32_t *h_channels,
                    int n_channels, int64_t F, int64_t C, int T, const float *d_tracks, const int32_t *d_ntracks,
                    const float *d_anchors, const void *d_det_score, int det_f64, const double *d_gt_overlap, float *d_conv_score)
{
    const int64_t foff[2] = {0, F};
    return vdet_tcn_tracks_batch(c, h_params, h_layers, n_layers, h_channels, n_channels, foff, 1, C, T, d_tracks, d_ntracks, d_anchors,
                                 d_det_score, det_f64, d_gt_overlap, d_conv_score);
}

int vdet_tcn_tracks_wide_batch(vdet_ctx *c, const float *h_params, const int32_t *h_layers, int n_layers, const int32_t *h_codes,
                               const int32_t *h_widths, const void *const *h_rows, const int32_t *h_dtypes, int n_inputs,
                               const int64_t *h_frame_off, int64_t V, int64_t C, int T, const float *d_tracks,
                               const int32_t *d_ntracks, const float *d_anchors, const void *d_det_score, int det_f64,
                               const double *d_gt_overlap, float *d_conv_score)
{
    if (!c) return VDET_EINVAL;
    if (!h_codes || !h_widths || !h_rows || !h_dtypes) return fail(c, VDET_EINVAL, "null buffer");
    if (n_inputs < 1 || n_inputs > kTcnMaxSegs) return fail(c, VDET_EINVAL, "1 to %d inputs", kTcnMaxSegs);
    TcnChannels ch{};
    TcnSeg segs[kTcnMaxSegs] = {};
    int64_t cin = 0;
    for (int i = 0; i < n_inputs; ++i) {
        TcnSeg &sg = segs[i];
        sg.c0 = (int32_t)cin;
        if (h_codes[i] == -1) {
            if (h_widths[i] < 1 || h_widths[i] > kTcnMaxChannels) return fail(c, VDET_EINVAL, "input %d: a wide blob has 1 to %d channels", i, kTcnMaxChannels);
            if (h_dtypes[i] < 0 || h_dtypes[i] >= kTcnRowTypes) return fail(c, VDET_EINVAL, "input %d: unknown row dtype %d", i, h_dtypes[i]);
            if (!h_rows[i]) return fail(c, VDET_EINVAL, "input %d: null rows", i);
            sg.rows = h_rows[i]; sg.width = h_widths[i]; sg.dtype = h_dtypes[i];
        } else {
            if (h_codes[i] < 0 || h_codes[i] >= kChCount) return fail(c, VDET_EINVAL, "unknown input channel code %d", h_codes[i]);
            if (h_widths[i] != 1) return fail(c, VDET_EINVAL, "input %d: an assembled channel has width 1", i);
            sg.width = 1; sg.xq = ch.n;
            ch.code[ch.n++] = h_codes[i];
        }
        cin += sg.width;
    }
    if (cin > kTcnMaxChannels) return fail(c, VDET_EINVAL, "a net has 1 to %d input channels", kTcnMaxChannels);
    return tcn_tracks_impl(c, h_params, h_layers, n_layers, ch, segs, n_inputs, (int)cin, h_frame_off, V, C, T, d_tracks, d_ntracks,
                           d_anchors, d_det_score, det_f64, d_gt_overlap, d_conv_score);
}

int vdet_tcn_tracks_wide(vdet_ctx *c, const float *h_params, const int32_t *h_layers, int n_layers, const int32_t *h_codes,
                         const int32_t *h_widths, const void *const *h_rows, const int32_t *h_dtypes, int n_inputs, int64_t F, int64_t C,
                         int T, const float *d_tracks, const int32_t *d_ntracks, const float *d_anchors, const void *d_det_score,
                         int det_f64, const double *d_gt_overlap, float *d_conv_score)
{
    const int64_t foff[2] = {0, F};
    return vdet_tcn_tracks_wide_batch(c, h_params, h_layers, n_layers, h_codes, h_widths, h_rows, h_dtypes, n_inputs, foff, 1, C, T,
                                      d_tracks, d_ntracks, d_anchors, d_det_score, det_f64, d_gt_overlap, d_conv_score);
}

int vdet_tcn_series_f32(vdet_ctx *c, const float *h_params, const int32_t *h_layers, int n_layers, int cin, const float *h_x,
                        const int64_t *h_off, int64_t T, float *h_out)
{
    if (!c) return VDET_EINVAL;
    if (T < 0 || (T && !h_off)) return fail(c, VDET_EINVAL, "bad series table");
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    TcnNet net;
    int rc = tcn_net_args(c, h_params, h_layers, n_layers, cin, net);
    if (rc) return rc;
    if (T == 0) return VDET_OK;
    if (h_off[0] != 0) return fail(c, VDET_EINVAL, "series offsets must start at 0");
    std::vector<int32_t> len((size_t)T);
    int64_t Lmax = 0;
    for (int64_t t = 0; t < T; ++t) {
        const int64_t l = h_off[t + 1] - h_off[t];
        if (l < 0 || l > 0x3FFFFFF0ll) return fail(c, VDET_EINVAL, "series offsets must not decrease");
        len[(size_t)t] = (int32_t)l;
        Lmax = std::max(Lmax, l);
    }
    const int64_t n = h_off[T];
    if (n == 0) return VDET_OK;
    if (!fits_upto(1ll << 40, {n, cin})) return fail(c, VDET_EINVAL, "too many series elements");
    if (!h_x || !h_out) return fail(c, VDET_EINVAL, "null buffer");
    if ((rc = upload(c, c->tmp[0], h_x, (size_t)n * cin * 4))) return rc;
    if ((rc = upload(c, c->tmp[1], h_off, (size_t)T * 8))) return rc;
    if ((rc = upload(c, c->tmp[2], len.data(), (size_t)T * 4))) return rc;
    HIPCHK(c, c->tmp[3].reserve((size_t)n * 4));
    if ((rc = tcn_launch_net(c, net, c->tmp[0].as<float>(), nullptr, c->tmp[1].as<int64_t>(), c->tmp[2].as<int32_t>(), T, Lmax,
                             c->tmp[3].as<float>())))
        return rc;
    HIPCHK(c, hipMemcpyAsync(h_out, c->tmp[3].p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, host_sync(c));
    return VDET_OK;
}

int vdet_tubelets_overlap_batch(vdet_ctx *c, const double *d_gt_boxes, const int32_t *d_gt_off, const int64_t *d_vid_meta, int K,
                                const int32_t *h_vid, const int64_t *h_frame_off, int64_t V, int64_t C, int T, const float *d_tracks,
                                const float *d_boxes, const int32_t *d_ntracks, const int32_t *h_col_slot, double *d_gt_overlap,
                                double *d_mean_iou, int32_t *d_gt)
{
    if (!c) return VDET_EINVAL;
    EvGt g;
    int rc = eval_gt_args(c, d_gt_boxes, d_gt_off, d_vid_meta, K, 0, 0.5, g);
    if (rc) return rc;
    Videos vs;
    if ((rc = read_videos(c, h_frame_off, V, 65535, &vs))) return rc;
    if (!h_vid || !h_col_slot) return fail(c, VDET_EINVAL, "null buffer");
    if (C < 1 || C > 65535 || T < 0 || !fits_upto(0x7FFFFFF0ll, {C, std::max(T, 1), vs.F})) return fail(c, VDET_EINVAL, "bad shape");
    if (T == 0) return VDET_OK;
    if (!d_tracks || !d_ntracks || !d_gt_overlap || !d_mean_iou || !d_gt) return fail(c, VDET_EINVAL, "null buffer");
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    // host tables: frame offsets [V+1] i64 | column slots [C] i32 | video table indices [V] i32.  One video travels in the
    // kernel arguments, so that videos of different lengths one after the other keep the resident table (the column slots)
    const bool one = V == 1;
    const size_t o_slot = one ? 0 : (size_t)(V + 1) * 8, o_vid = o_slot + (size_t)C * 4;
    std::vector<char> tab(o_vid + (one ? 0 : (size_t)V * 4));
    if (!one) memcpy(tab.data(), h_frame_off, o_slot);
    memcpy(tab.data() + o_slot, h_col_slot, (size_t)C * 4);
    if (!one) memcpy(tab.data() + o_vid, h_vid, (size_t)V * 4);
    if ((rc = stage_table(c, c->tcn_ovtab, tab.data(), tab.size()))) return rc;
    const char *tb = c->tcn_ovtab.dev.as<char>();
    {
        StageTimer tm(c, ST_OTHER);
        hipLaunchKernelGGL(tubelets_overlap_kernel, dim3((unsigned)(C * T), (unsigned)V), dim3(64), 0, c->stream, g,
                           one ? (const int64_t *)nullptr : reinterpret_cast<const int64_t *>(tb), vs.F,
                           one ? (const int32_t *)nullptr : reinterpret_cast<const int32_t *>(tb + o_vid), h_vid[0], (int)C, T,
                           d_tracks, d_boxes, d_ntracks, reinterpret_cast<const int32_t *>(tb + o_slot), d_gt_overlap, d_mean_iou, d_gt);
    }
    HIPCHK(c, hipGetLastError());
    return VDET_OK;
}

int vdet_tubelets_overlap(vdet_ctx *c, const double *d_gt_boxes, const int32_t *d_gt_off, const int64_t *d_vid_meta, int K, int vid,
                          int64_t F, int64_t C, int T, const float *d_tracks, const float *d_boxes, const int32_t *d_ntracks,
                          const int32_t *h_col_slot, double *d_gt_overlap, double *d_mean_iou, int32_t *d_gt)
{
    const int64_t foff[2] = {0, F};
    return vdet_tubelets_overlap_batch(c, d_gt_boxes, d_gt_off, d_vid_meta, K, &vid, foff, 1, C, T, d_tracks, d_boxes, d_ntracks,
                                       h_col_slot, d_gt_overlap, d_mean_iou, d_gt);
}


// ---------------------------------------------------------------------------------------------
// Device interpolation (interp_kernels.hpp)
// ---------------------------------------------------------------------------------------------
int vdet_interp_tracks_batch(vdet_ctx *c, const int64_t *h_sframe_off, const int64_t *h_frame_off, int64_t V, const int32_t *h_frames,
                             int64_t C, int T, const float *d_tracks, const float *d_boxes, const int32_t *d_ntracks,
                             const float *d_anchors, const void *const *h_series, int n_series, int series_f64, float *d_tracks_out,
                             double *d_boxes64, float *d_tboxes, double *d_series_out, double *d_anchor, float *d_anchors_out)
{
    if (!c) return VDET_EINVAL;
    Videos sampled, dense;
    int rc = read_videos(c, h_sframe_off, V, 65535, &sampled);
    if (rc) return rc;
    if ((rc = read_videos(c, h_frame_off, V, 65535, &dense))) return rc;
    const int64_t Fst = sampled.F, Ft = dense.F;
    if (C < 1 || T < 0 || !fits_upto(0x7FFFFFF0ll, {C, std::max(T, 1)})) return fail(c, VDET_EINVAL, "bad shape");
    if (n_series < 0 || n_series > kInterpMaxSeries) return fail(c, VDET_EINVAL, "0 to %d series", kInterpMaxSeries);
    if (!fits_upto(0x7FFFFFF0ll, {C, std::max(T, 1), Ft}) || !fits_upto(0x7FFFFFF0ll, {C, std::max(T, 1), Fst}))
        return fail(c, VDET_EINVAL, "too many tubelet boxes (C*T*F must stay below 2^31)");
    for (int64_t v = 0; v < V; ++v) {
        const int64_t s0 = h_sframe_off[v], fs = h_sframe_off[v + 1] - s0, f = h_frame_off[v + 1] - h_frame_off[v];
        if (!h_frames) {
            if (f < fs) return fail(c, VDET_EINVAL, "video %lld: %lld dense frames for %lld rows", (long long)v, (long long)f, (long long)fs);
            continue;
        }
        for (int64_t i = 0; i < fs; ++i) {
            const int64_t x = h_frames[s0 + i];
            if (x < 1 || (i && x <= h_frames[s0 + i - 1]))
                return fail(c, VDET_EINVAL, "video %lld: frames must be >= 1 and strictly ascending", (long long)v);
        }
        if (h_frames[s0 + fs - 1] > f)
            return fail(c, VDET_EINVAL, "video %lld: frame %d lies beyond its %lld dense frames", (long long)v, (int)h_frames[s0 + fs - 1], (long long)f);
    }
    if (T == 0) return VDET_OK;
    if (!d_tracks || !d_ntracks || !d_anchors || !d_tracks_out || !d_boxes64 || !d_tboxes || !d_anchor || !d_anchors_out ||
        (n_series && (!h_series || !d_series_out)))
        return fail(c, VDET_EINVAL, "null buffer");
    InterpArgs a{};
    for (int q = 0; q < n_series; ++q) {
        if (!h_series[q]) return fail(c, VDET_EINVAL, "null buffer");
        a.series[q] = h_series[q];
    }
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    // host tables: sampled offsets [V+1] i64 | dense offsets [V+1] i64 (both only for V > 1) | frames [Fs] i32 (when given).
    // One video on an identity axis travels in the kernel arguments alone.
    const bool many = V > 1;
    const size_t o_fr = many ? (size_t)(V + 1) * 16 : 0;
    if (many || h_frames) {
        std::vector<char> tab(o_fr + (h_frames ? (size_t)Fst * 4 : 0));
        if (many) {
            memcpy(tab.data(), h_sframe_off, (size_t)(V + 1) * 8);
            memcpy(tab.data() + (size_t)(V + 1) * 8, h_frame_off, (size_t)(V + 1) * 8);
        }
        if (h_frames) memcpy(tab.data() + o_fr, h_frames, (size_t)Fst * 4);
        if ((rc = stage_table(c, c->interp_tab, tab.data(), tab.size()))) return rc;
        const char *tb = c->interp_tab.dev.as<char>();
        if (many) {
            a.soff = reinterpret_cast<const int64_t *>(tb);
            a.doff = a.soff + (V + 1);
        }
        if (h_frames) a.frames = reinterpret_cast<const int32_t *>(tb + o_fr);
    }
    a.tracks = d_tracks; a.boxes = d_boxes; a.ntracks = d_ntracks; a.anchors = d_anchors;
    a.nser = n_series; a.oseries = d_series_out; a.N = C * T * Ft;
    a.Fs1 = (int)Fst; a.F1 = (int)Ft; a.C = (int)C; a.T = T;
    a.otracks = d_tracks_out; a.boxes64 = d_boxes64; a.tboxes = d_tboxes; a.oanchor = d_anchor; a.oanchors = d_anchors_out;
    {
        StageTimer tm(c, ST_OTHER);
        const dim3 grid((unsigned)(C * T), (unsigned)V);
#define VDET_INTERP_LAUNCH(N_)                                                                              \
    case N_:                                                                                                \
        if (series_f64) hipLaunchKernelGGL((interp_tracks_kernel<N_, true>), grid, dim3(64), 0, c->stream, a);  \
        else hipLaunchKernelGGL((interp_tracks_kernel<N_, false>), grid, dim3(64), 0, c->stream, a);            \
        break;
        switch (n_series) {
            VDET_INTERP_LAUNCH(0) VDET_INTERP_LAUNCH(1) VDET_INTERP_LAUNCH(2) VDET_INTERP_LAUNCH(3) VDET_INTERP_LAUNCH(4)
        }
#undef VDET_INTERP_LAUNCH
    }
    HIPCHK(c, hipGetLastError());
    return VDET_OK;
}

int vdet_interp_tracks(vdet_ctx *c, int64_t Fs, int64_t F, const int32_t *h_frames, int64_t C, int T, const float *d_tracks,
                       const float *d_boxes, const int32_t *d_ntracks, const float *d_anchors, const void *const *h_series,
                       int n_series, int series_f64, float *d_tracks_out, double *d_boxes64, float *d_tboxes,
                       double *d_series_out, double *d_anchor, float *d_anchors_out)
{
    const int64_t soff[2] = {0, Fs}, doff[2] = {0, F};
    return vdet_interp_tracks_batch(c, soff, doff, 1, h_frames, C, T, d_tracks, d_boxes, d_ntracks, d_anchors, h_series, n_series,
                                    series_f64, d_tracks_out, d_boxes64, d_tboxes, d_series_out, d_anchor, d_anchors_out);
}

// ---------------------------------------------------------------------------------------------
// Device anchor route (anchor_kernels.hpp)
// ---------------------------------------------------------------------------------------------
int vdet_anchor_argmax_f64(vdet_ctx *c, const double *h_anchor_boxes, const int32_t *h_group, int64_t N, const double *h_det_boxes,
                           const int64_t *h_group_off, int64_t G, int64_t *h_best)
{
    if (!c || N < 0 || G < 0) return VDET_EINVAL;
    if (N == 0) return VDET_OK;
    if (N > 0x7FFFFFF0ll) return fail(c, VDET_EINVAL, "too many anchors");
    if (!h_anchor_boxes || !h_group || !h_group_off || !h_best || G == 0) return fail(c, VDET_EINVAL, "null buffer");
    if (h_group_off[0] != 0) return fail(c, VDET_EINVAL, "group_off must start at 0");
    for (int64_t g = 0; g < G; ++g)
        if (h_group_off[g + 1] < h_group_off[g]) return fail(c, VDET_EINVAL, "group_off must not decrease");
    const int64_t M = h_group_off[G];
    if (M && !h_det_boxes) return fail(c, VDET_EINVAL, "null buffer");
    for (int64_t n = 0; n < N; ++n)
        if (h_group[n] < 0 || h_group[n] >= G) return fail(c, VDET_EINVAL, "anchor frame slot out of range");
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    int rc;
    if ((rc = upload(c, c->tmp[0], h_anchor_boxes, (size_t)N * 32))) return rc;
    if ((rc = upload(c, c->tmp[1], h_group, (size_t)N * 4))) return rc;
    if ((rc = upload(c, c->tmp[2], h_det_boxes, (size_t)M * 32))) return rc;
    if ((rc = upload(c, c->tmp[3], h_group_off, (size_t)(G + 1) * 8))) return rc;
    HIPCHK(c, c->tmp[4].reserve((size_t)N * 8));
    {
        StageTimer tm(c, ST_OTHER);
        hipLaunchKernelGGL(anchor_argmax_f64_kernel, dim3((unsigned)N), dim3(kAnchorLT), 0, c->stream, c->tmp[0].as<double>(),
                           c->tmp[1].as<int32_t>(), c->tmp[2].as<double>(), c->tmp[3].as<int64_t>(), c->tmp[4].as<int64_t>());
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h_best, c->tmp[4].p, (size_t)N * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, host_sync(c));
    return VDET_OK;
}

int vdet_top_anchors(vdet_ctx *c, const float *d_boxes, const float *d_scores, int64_t F, int64_t B, int64_t C, int top_num,
                     int mode, int use_score_thresh, double score_thresh, const int64_t *h_frame_off, int64_t V,
                     int32_t *d_anchor_frames, float *d_anchor_boxes, float *d_anchor_scores, int32_t *d_anchor_index)
{
    if (!c) return VDET_EINVAL;
    if (mode != 0 && mode != 1) return fail(c, VDET_EINVAL, "mode must be 0 (video) or 1 (frame)");
    if (F <= 0 || B <= 0 || C <= 0) return fail(c, VDET_EINVAL, "bad shape");
    if (top_num < 1) return fail(c, VDET_EINVAL, "top_num must be at least 1");
    if (mode == 0 && top_num > kTopaMaxT) return fail(c, VDET_EINVAL, "top_num = %d; the limit is %d per class", top_num, kTopaMaxT);
    if (mode == 1 && top_num > kTopaMaxTFrame) return fail(c, VDET_EINVAL, "top_num = %d; the limit is %d per frame and class", top_num, kTopaMaxTFrame);
    if (mode == 1 && h_frame_off) return fail(c, VDET_EINVAL, "frame mode has no batch form");
    if (B > 32767) return fail(c, VDET_EINVAL, "B = %lld boxes per frame; the limit is 32767", (long long)B);
    if (!fits_upto(0x7FFFFFF0ll, {F, B})) return fail(c, VDET_EINVAL, "volume too large (F*B must stay below 2^31 - 16)");
    if (!d_boxes || !d_scores || !d_anchor_frames || !d_anchor_boxes || !d_anchor_scores || !d_anchor_index) return fail(c, VDET_EINVAL, "null buffer");
    if (((uintptr_t)d_boxes & 15) != 0 || ((uintptr_t)d_anchor_boxes & 15) != 0) return fail(c, VDET_EINVAL, "d_boxes and d_anchor_boxes must be 16-byte aligned");
    Videos vs;
    int rc = read_videos_or_one(c, h_frame_off, V, F, 65535, &vs);
    if (rc) return rc;
    int64_t Fmax = vs.Fmax, nv = vs.V;
    if (mode == 1) {            // (no offsets: every frame is a video of its own)
        if (F > 65535) return fail(c, VDET_EINVAL, "frame mode: at most 65535 frames");
        nv = F; Fmax = 1;
    }
    const int T = top_num;
    const int64_t nseg = (Fmax * B + kTopaRows - 1) / kTopaRows, ctiles = (C + 63) / 64;
    if (!fits_upto(0x7FFFFFF0ll, {nv, C, T}) || !fits_upto(0x7FFFFFF0ll, {nv, nseg, C}) || ctiles > 65535) return fail(c, VDET_EINVAL, "too many slots");
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    if (h_frame_off && (rc = stage_video_table(c, c->anchor_tab, vs))) return rc;
    const size_t hist_bytes = (size_t)(nv * C) * 256 * 4;
    if (hist_bytes > c->topa_hist.cap) c->topa_hist_clean = false;
    HIPCHK(c, c->topa_hist.reserve(hist_bytes));
    HIPCHK(c, c->topa_state.reserve((size_t)(nv * C) * 8));
    HIPCHK(c, c->topa_cnt.reserve((size_t)(nv * nseg * C) * 8));
    HIPCHK(c, c->topa_nrec.reserve((size_t)(nv * C) * 4));
    HIPCHK(c, c->topa_rec.reserve((size_t)(nv * C) * T * 8));
    if (!c->topa_hist_clean) HIPCHK(c, hipMemsetAsync(c->topa_hist.p, 0, c->topa_hist.cap, c->stream));
    c->topa_hist_clean = false;
    TopaArgs a{};
    a.scores = d_scores; a.boxes = reinterpret_cast<const float4 *>(d_boxes);
    a.vids = h_frame_off ? c->anchor_tab.dev.as<VidDesc>() : nullptr;
    a.Fu = mode == 1 ? 1 : (int)F;
    a.V = (int)nv; a.B = (int)B; a.C = (int)C; a.T = T;
    a.use_thr = use_score_thresh ? 1 : 0; a.thr = (float)score_thresh;
    a.nseg = (int)nseg; a.frame_mode = mode;
    a.hist = c->topa_hist.as<uint32_t>(); a.state = c->topa_state.as<uint2>(); a.cnt = c->topa_cnt.as<uint2>();
    a.nrec = c->topa_nrec.as<uint32_t>(); a.rec = c->topa_rec.as<unsigned long long>();
    a.ovs = mode == 1 ? T : C * (int64_t)T; a.ocs = mode == 1 ? F * (int64_t)T : T;
    a.oframes = d_anchor_frames; a.oboxes = reinterpret_cast<float4 *>(d_anchor_boxes); a.oscores = d_anchor_scores;
    a.oindex = d_anchor_index;
    const dim3 ghist((unsigned)((nseg + kTopaHistLT / 64 - 1) / (kTopaHistLT / 64)), (unsigned)ctiles, (unsigned)nv);
    const dim3 gseg((unsigned)((nseg + kTopaLT / 64 - 1) / (kTopaLT / 64)), (unsigned)ctiles, (unsigned)nv);
    const dim3 gcls((unsigned)C, (unsigned)nv);
    {
        StageTimer tm(c, ST_TPICK);
        for (int pass = 0; pass < 4; ++pass) {
            hipLaunchKernelGGL(topa_hist_kernel, ghist, dim3(kTopaHistLT), 0, c->stream, a, pass);
            hipLaunchKernelGGL(topa_select_kernel, gcls, dim3(256), 0, c->stream, a, pass);
        }
        hipLaunchKernelGGL(topa_count_kernel, gseg, dim3(kTopaLT), 0, c->stream, a);
        hipLaunchKernelGGL(topa_prefix_kernel, dim3((unsigned)ctiles, (unsigned)nv), dim3(1024), 0, c->stream, a);
        hipLaunchKernelGGL(topa_gather_kernel, gseg, dim3(kTopaLT), 0, c->stream, a);
        hipLaunchKernelGGL(topa_emit_kernel, gcls, dim3(kTopaLT), 0, c->stream, a, (int)pow2ceil((uint32_t)T));
    }
    HIPCHK(c, hipGetLastError());
    c->topa_hist_clean = true;
    return VDET_OK;
}

int vdet_track_from_anchors_batch(vdet_ctx *c, const float *d_boxes, const int64_t *h_frame_off, int64_t V, int64_t B,
                                  const int32_t *d_anchor_frames, const float *d_anchor_boxes, const float *d_anchor_scores,
                                  int64_t C, int T, double link_thres, int max_frames, float *d_tracks, float *d_anchors,
                                  int32_t *d_ntracks)
{
    if (!c) return VDET_EINVAL;
    if (B <= 0 || C <= 0 || T < 0) return fail(c, VDET_EINVAL, "bad shape");
    if (B > 32767) return fail(c, VDET_EINVAL, "at most 32767 boxes per frame");
    Videos vs;
    int rc = read_videos(c, h_frame_off, V, 65535, &vs);
    if (rc) return rc;
    if (!fits_upto(0x7FFFFFF0ll, {vs.F, B}) || !fits_upto(0x7FFFFFF0ll, {C, std::max(T, 1), vs.F}) || !fits_upto(0x7FFFFFF0ll, {V, C, std::max(T, 1)}))
        return fail(c, VDET_EINVAL, "volume too large (F*B, C*T*F and V*C*T must stay below 2^31)");
    if (!d_boxes || !d_ntracks || (T && (!d_anchor_frames || !d_anchor_boxes || !d_tracks || !d_anchors))) return fail(c, VDET_EINVAL, "null buffer");
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    if (T == 0) {
        HIPCHK(c, hipMemsetAsync(d_ntracks, 0, (size_t)(V * C) * 4, c->stream));
        return VDET_OK;
    }
    // one video travels in the kernel arguments alone; more run the batch kernel on the per-video table
    AnchorLinkArgs a{};
    if ((rc = video_table(c, c->anchor_tab, vs, &a.vids))) return rc;
    a.boxes = reinterpret_cast<const float4 *>(d_boxes);
    a.F = (int)vs.F; a.B = (int)B; a.C = (int)(V * C); a.T = T;
    a.cls = a.vids ? (int)C : 0;
    a.aframes = d_anchor_frames; a.aboxes = d_anchor_boxes; a.ascores = d_anchor_scores;
    a.link_t32 = thresh_to_f32(link_thres);
    a.reach = chain_reach(max_frames, (int)vs.Fmax);
    a.tracks = d_tracks; a.anchors = d_anchors; a.ntracks = d_ntracks;
    a.status = &c->d_cnt->status;
    {
        StageTimer tm(c, ST_TLINK);
        const dim3 grid((unsigned)(V * C * T), 2);
        if (a.vids) hipLaunchKernelGGL(anchor_link_kernel<true>, grid, dim3(kAnchorLT), 0, c->stream, a);
        else hipLaunchKernelGGL(anchor_link_kernel<false>, grid, dim3(kAnchorLT), 0, c->stream, a);
    }
    HIPCHK(c, hipGetLastError());
    return VDET_OK;
}

int vdet_anchor_propagate_tracks_batch(vdet_ctx *c, const float *d_tracks, const int32_t *d_ntracks, const float *d_anchors,
                                       const float *d_boxes, const float *d_scores, const int64_t *h_frame_off, int64_t V,
                                       int64_t B, int64_t C, int T, double *d_det_score, int32_t *d_best)
{
    if (!c) return VDET_EINVAL;
    if (B <= 0 || C <= 0 || T < 0) return fail(c, VDET_EINVAL, "bad shape");
    if (B > 32767) return fail(c, VDET_EINVAL, "at most 32767 boxes per frame");
    Videos vs;
    int rc = read_videos(c, h_frame_off, V, 65535, &vs);
    if (rc) return rc;
    if (!fits_upto(0x7FFFFFF0ll, {vs.F, B}) || !fits_upto(0x7FFFFFF0ll, {C, std::max(T, 1), vs.F}) || !fits_upto(0x7FFFFFF0ll, {V, C, std::max(T, 1)}))
        return fail(c, VDET_EINVAL, "volume too large (F*B, C*T*F and V*C*T must stay below 2^31)");
    if (T == 0) return VDET_OK;
    if (!d_tracks || !d_ntracks || !d_anchors || !d_boxes || !d_scores || !d_det_score || !d_best) return fail(c, VDET_EINVAL, "null buffer");
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    const VidDesc *vids = nullptr;      // (one video travels in the kernel arguments alone)
    if ((rc = video_table(c, c->anchor_tab, vs, &vids))) return rc;
    {
        StageTimer tm(c, ST_OTHER);
        const auto kernel = vids ? anchor_propagate_kernel<true> : anchor_propagate_kernel<false>;
        hipLaunchKernelGGL(kernel, dim3((unsigned)(V * C * T)), dim3(kAnchorLT), 0, c->stream, d_tracks, d_ntracks, d_anchors, d_boxes,
                           d_scores, (int)vs.F, (int)B, (int)(V * C), T, d_det_score, d_best, &c->d_cnt->status, vids, vids ? (int)C : 0);
    }
    HIPCHK(c, hipGetLastError());
    return VDET_OK;
}

int vdet_track_from_anchors(vdet_ctx *c, const float *d_boxes, int64_t F, int64_t B, const int32_t *d_anchor_frames,
                            const float *d_anchor_boxes, const float *d_anchor_scores, int64_t C, int T, double link_thres,
                            int max_frames, float *d_tracks, float *d_anchors, int32_t *d_ntracks)
{
    const int64_t off[2] = {0, F};
    return vdet_track_from_anchors_batch(c, d_boxes, off, 1, B, d_anchor_frames, d_anchor_boxes, d_anchor_scores, C, T, link_thres,
                                         max_frames, d_tracks, d_anchors, d_ntracks);
}

int vdet_anchor_propagate_tracks(vdet_ctx *c, const float *d_tracks, const int32_t *d_ntracks, const float *d_anchors,
                                 const float *d_boxes, const float *d_scores, int64_t F, int64_t B, int64_t C, int T,
                                 double *d_det_score, int32_t *d_best)
{
    const int64_t off[2] = {0, F};
    return vdet_anchor_propagate_tracks_batch(c, d_tracks, d_ntracks, d_anchors, d_boxes, d_scores, off, 1, B, C, T, d_det_score, d_best);
}

// ---------------------------------------------------------------------------------------------
// Device merge of two tubelet sets (merge_kernels.hpp)
// ---------------------------------------------------------------------------------------------
int vdet_merge_tracks_batch(vdet_ctx *c, int scheme, const int64_t *h_frame_off, int64_t V, int64_t C, int Ta, int Tb,
                            const float *d_tracks_a, const int32_t *d_ntracks_a, const float *d_anchors_a, const float *d_tboxes_a,
                            const float *d_tracks_b, const int32_t *d_ntracks_b, const float *d_anchors_b, const float *d_tboxes_b,
                            const double *const *h_series_a, const double *const *h_series_b, int n_series, float *d_tracks_out,
                            int32_t *d_ntracks_out, float *d_anchors_out, float *d_tboxes_out, double *d_series_out,
                            uint8_t *d_from_b)
{
    if (!c) return VDET_EINVAL;
    if (scheme != VDET_MERGE_COMBINE && scheme != VDET_MERGE_MAX) return fail(c, VDET_EINVAL, "scheme must be VDET_MERGE_COMBINE or VDET_MERGE_MAX");
    if (n_series < 1 || n_series > kMergeMaxSeries) return fail(c, VDET_EINVAL, "1 to %d series (series 0 is det_score)", kMergeMaxSeries);
    if (C < 1 || Ta < 0 || Tb < 0) return fail(c, VDET_EINVAL, "bad shape");
    Videos vs;
    int rc = read_videos(c, h_frame_off, V, 65535, &vs);
    if (rc) return rc;
    const int64_t To = scheme == VDET_MERGE_COMBINE ? (int64_t)Ta + Tb : Ta, Tmax = std::max<int64_t>(std::max<int64_t>(To, Tb), 1);
    if (!fits_below(0x7FFFFFF0ll, {C, Tmax, vs.F}) || !fits_below(0x7FFFFFF0ll, {V, C, Tmax}))
        return fail(c, VDET_EINVAL, "too many tubelet boxes (C*T*F must stay below 2^31 - 16 for Ta, Tb and the output's T)");
    if (!d_ntracks_a || !d_ntracks_b || !d_ntracks_out) return fail(c, VDET_EINVAL, "null buffer");
    const bool tbx = d_tboxes_out != nullptr;
    if ((Ta && (d_tboxes_a != nullptr) != tbx) || (Tb && (d_tboxes_b != nullptr) != tbx))
        return fail(c, VDET_EINVAL, "tboxes: both sets and the output, or none of them");
    if ((Ta && (!d_tracks_a || !d_anchors_a || !h_series_a)) || (Tb && (!d_tracks_b || !d_anchors_b || !h_series_b)) ||
        (To && (!d_tracks_out || !d_anchors_out || !d_series_out)) || (scheme == VDET_MERGE_MAX && To && !d_from_b))
        return fail(c, VDET_EINVAL, "null buffer");
    MergeArgs g{};
    for (int q = 0; q < n_series; ++q) {
        if ((Ta && !h_series_a[q]) || (Tb && !h_series_b[q])) return fail(c, VDET_EINVAL, "null buffer");
        g.a.series[q] = Ta ? h_series_a[q] : nullptr;
        g.b.series[q] = Tb ? h_series_b[q] : nullptr;
    }
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    if (To == 0) {      // no slot to write: the counts alone ('combine': 0 + 0, 'max': a's, clamped to Ta = 0)
        HIPCHK(c, hipMemsetAsync(d_ntracks_out, 0, (size_t)(V * C) * 4, c->stream));
        return VDET_OK;
    }
    if ((rc = video_table(c, c->anchor_tab, vs, &g.vids))) return rc;
    g.a.tracks = d_tracks_a; g.a.ntracks = d_ntracks_a; g.a.anchors = d_anchors_a; g.a.tboxes = d_tboxes_a; g.a.T = Ta;
    g.b.tracks = d_tracks_b; g.b.ntracks = d_ntracks_b; g.b.anchors = d_anchors_b; g.b.tboxes = d_tboxes_b; g.b.T = Tb;
    g.F = (int)vs.F; g.C = (int)C; g.nser = n_series; g.To = (int)To;
    g.otracks = d_tracks_out; g.ontracks = d_ntracks_out; g.oanchors = d_anchors_out; g.otboxes = d_tboxes_out;
    g.oseries = d_series_out; g.oN = C * To * vs.F; g.from_b = d_from_b; g.status = &c->d_cnt->status;
    {
        StageTimer tm(c, ST_OTHER);
        const dim3 grid((unsigned)((C * To + kMergeWaves - 1) / kMergeWaves), (unsigned)V);
        if (scheme == VDET_MERGE_COMBINE) hipLaunchKernelGGL(merge_combine_kernel, grid, dim3(kMergeLT), 0, c->stream, g);
        else hipLaunchKernelGGL(merge_max_kernel, grid, dim3(kMergeLT), 0, c->stream, g);
    }
    HIPCHK(c, hipGetLastError());
    return VDET_OK;
}

int vdet_merge_tracks(vdet_ctx *c, int scheme, int64_t F, int64_t C, int Ta, int Tb,
                      const float *d_tracks_a, const int32_t *d_ntracks_a, const float *d_anchors_a, const float *d_tboxes_a,
                      const float *d_tracks_b, const int32_t *d_ntracks_b, const float *d_anchors_b, const float *d_tboxes_b,
                      const double *const *h_series_a, const double *const *h_series_b, int n_series, float *d_tracks_out,
                      int32_t *d_ntracks_out, float *d_anchors_out, float *d_tboxes_out, double *d_series_out, uint8_t *d_from_b)
{
    const int64_t off[2] = {0, F};
    return vdet_merge_tracks_batch(c, scheme, off, 1, C, Ta, Tb, d_tracks_a, d_ntracks_a, d_anchors_a, d_tboxes_a, d_tracks_b,
                                   d_ntracks_b, d_anchors_b, d_tboxes_b, h_series_a, h_series_b, n_series, d_tracks_out,
                                   d_ntracks_out, d_anchors_out, d_tboxes_out, d_series_out, d_from_b);
}

// ---------------------------------------------------------------------------------------------
// Per-frame NMS of tubelets with still-image detections (tracknms_kernels.hpp)
// ---------------------------------------------------------------------------------------------
// the checks of vdet_nms_tracks[_batch] and its kernel arguments, shared with vdet_soft_nms_tracks[_batch] and
// vdet_vote_nms_tracks[_batch]: nothing is launched, nothing written; vs = the videos as read
static int tracknms_args(vdet_ctx *c, const int64_t *h_frame_off, int64_t V, int64_t C, int T, const float *d_tracks,
                         const int32_t *d_ntracks, const void *d_score, int score_f64, const float *d_tboxes, const float *d_boxes,
                         const float *d_scores, int64_t B, const int32_t *d_keep_idx, const int32_t *d_keep_cnt, int64_t cap,
                         int top_still, double thresh, int R, float *d_tracks_out, double *d_score_out, int32_t *d_src_out,
                         int32_t *d_cnt_out, int32_t *d_ntracks_out, Videos &vs, TrackNmsArgs &g)
{
    if (C < 1 || T < 0 || top_still < 0) return fail(c, VDET_EINVAL, "bad shape");
    int rc = read_videos(c, h_frame_off, V, 65535, &vs);
    if (rc) return rc;
    const int64_t F = vs.F;
    if ((int64_t)top_still + T > kTnMaxList)
        return fail(c, VDET_EINVAL, "top_still + T = %lld candidates per (frame, class); the limit is %d", (long long)top_still + T, kTnMaxList);
    if (R < 1 || R > kTnMaxList) return fail(c, VDET_EINVAL, "R = %d output rows per (frame, class); 1 .. %d", R, kTnMaxList);
    if (!fits_below(0x7FFFFFF0ll, {C, R, F}) || !fits_below(0x7FFFFFF0ll, {C, T, F}) || !fits_below(0x7FFFFFF0ll, {V, C}))
        return fail(c, VDET_EINVAL, "too many tubelet boxes (C*R*F and C*T*F must stay below 2^31 - 16)");
    if (top_still > 0) {
        if (B < 1 || B > 32767) return fail(c, VDET_EINVAL, "B = %lld boxes per frame; 1 .. 32767", (long long)B);
        if (cap < 1 || cap > 0x7FFFFFF0ll || !fits_below(1ll << 40, {F, C, cap})) return fail(c, VDET_EINVAL, "bad keep-list capacity");
        if (!d_boxes || !d_scores || !d_keep_idx || !d_keep_cnt) return fail(c, VDET_EINVAL, "null buffer (top_still > 0 needs the still-image source)");
        if (((uintptr_t)d_boxes & 15) != 0) return fail(c, VDET_EINVAL, "d_boxes must be 16-byte aligned");
    }
    if (T > 0 && (!d_tracks || !d_ntracks || !d_score)) return fail(c, VDET_EINVAL, "null buffer");
    if (T > 0 && d_tboxes && ((uintptr_t)d_tboxes & 15) != 0) return fail(c, VDET_EINVAL, "d_tboxes must be 16-byte aligned");
    if (!d_tracks_out || !d_score_out || !d_src_out || !d_cnt_out || !d_ntracks_out) return fail(c, VDET_EINVAL, "null buffer");
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    if ((rc = video_table(c, c->anchor_tab, vs, &g.vids))) return rc;
    g.tracks = d_tracks; g.ntracks = d_ntracks; g.score = d_score; g.tboxes = T > 0 ? reinterpret_cast<const float4 *>(d_tboxes) : nullptr;
    g.boxes = reinterpret_cast<const float4 *>(d_boxes); g.scores = d_scores; g.keep_idx = d_keep_idx; g.keep_cnt = d_keep_cnt;
    g.F = (int)F; g.Ftot = (int)F; g.C = (int)C; g.T = T; g.B = (int)B; g.cap = (int)cap; g.top_still = top_still; g.R = R;
    g.nmax = top_still + T; g.score_f64 = score_f64 ? 1 : 0; g.t32 = thresh_to_f32(thresh);
    g.otracks = d_tracks_out; g.oscore = d_score_out; g.osrc = d_src_out; g.ocnt = d_cnt_out; g.ontracks = d_ntracks_out;
    g.status = &c->d_cnt->status;
    return VDET_OK;
}

extern "C++" {
// the launch tail of the three rules: args = what the kernel takes, g = its list part.  The LDS of a wave follows the call's own
// top_still + T; as many waves per workgroup (4, 2, 1) as stay BELOW 64 KiB
template <typename Args>
static int tracknms_launch(vdet_ctx *c, const Args &args, const TrackNmsArgs &g, const Videos &vs, void (*kernel)(Args), int bytes_per_cand)
{
    int waves = 4;
    // (the hard NMS never meets the bound itself: 65536 is divisible by neither 4 * 24 nor 2 * 24)
    while (waves > 1 && (size_t)waves * g.nmax * bytes_per_cand >= 65536) waves >>= 1;
    HIPCHK(c, hipMemsetAsync(g.ontracks, 0, (size_t)(vs.V * g.C) * 4, c->stream));
    {
        StageTimer tm(c, ST_OTHER);
        const dim3 grid((unsigned)(((int64_t)g.C * vs.Fmax + waves - 1) / waves), (unsigned)vs.V);
        hipLaunchKernelGGL(kernel, grid, dim3(64 * waves), (size_t)waves * g.nmax * bytes_per_cand, c->stream, args);
    }
    HIPCHK(c, hipGetLastError());
    return VDET_OK;
}
}  // extern "C++"

int vdet_nms_tracks_batch(vdet_ctx *c, const int64_t *h_frame_off, int64_t V, int64_t C, int T, const float *d_tracks,
                          const int32_t *d_ntracks, const void *d_score, int score_f64, const float *d_tboxes, const float *d_boxes,
                          const float *d_scores, int64_t B, const int32_t *d_keep_idx, const int32_t *d_keep_cnt, int64_t cap,
                          int top_still, double thresh, int R, float *d_tracks_out, double *d_score_out, int32_t *d_src_out,
                          int32_t *d_cnt_out, int32_t *d_ntracks_out)
{
    if (!c) return VDET_EINVAL;
    Videos vs;
    TrackNmsArgs g{};
    const int rc = tracknms_args(c, h_frame_off, V, C, T, d_tracks, d_ntracks, d_score, score_f64, d_tboxes, d_boxes, d_scores, B,
                                 d_keep_idx, d_keep_cnt, cap, top_still, thresh, R, d_tracks_out, d_score_out, d_src_out, d_cnt_out,
                                 d_ntracks_out, vs, g);
    if (rc) return rc;
    return tracknms_launch(c, g, g, vs, tracknms_kernel, kTnBytesPerCand);
}

int vdet_nms_tracks(vdet_ctx *c, int64_t F, int64_t C, int T, const float *d_tracks, const int32_t *d_ntracks, const void *d_score,
                    int score_f64, const float *d_tboxes, const float *d_boxes, const float *d_scores, int64_t B,
                    const int32_t *d_keep_idx, const int32_t *d_keep_cnt, int64_t cap, int top_still, double thresh, int R,
                    float *d_tracks_out, double *d_score_out, int32_t *d_src_out, int32_t *d_cnt_out, int32_t *d_ntracks_out)
{
    const int64_t off[2] = {0, F};
    return vdet_nms_tracks_batch(c, off, 1, C, T, d_tracks, d_ntracks, d_score, score_f64, d_tboxes, d_boxes, d_scores, B, d_keep_idx,
                                 d_keep_cnt, cap, top_still, thresh, R, d_tracks_out, d_score_out, d_src_out, d_cnt_out,
                                 d_ntracks_out);
}

// ---------------------------------------------------------------------------------------------
// Soft-NMS of the same lists (softnms_kernels.hpp)
// ---------------------------------------------------------------------------------------------
int vdet_soft_nms_tracks_batch(vdet_ctx *c, const int64_t *h_frame_off, int64_t V, int64_t C, int T, const float *d_tracks,
                               const int32_t *d_ntracks, const void *d_score, int score_f64, const float *d_tboxes,
                               const float *d_boxes, const float *d_scores, int64_t B, const int32_t *d_keep_idx,
                               const int32_t *d_keep_cnt, int64_t cap, int top_still, double thresh, int R, int method, double sigma,
                               double min_score, float *d_tracks_out, double *d_score_out, int32_t *d_src_out, int32_t *d_cnt_out,
                               int32_t *d_ntracks_out, double *d_score0_out)
{
    if (!c) return VDET_EINVAL;
    if (method != kSnLinear && method != kSnGauss) return fail(c, VDET_EINVAL, "method = %d; 0 (linear) or 1 (gauss)", method);
    if (!std::isfinite(sigma) || !(sigma >= kSnSigmaMin))
        return fail(c, VDET_EINVAL, "sigma = %g; finite and at least 1/64 (the Gaussian weight's argument stays in [-64, 0])", sigma);
    if (thresh != thresh || min_score != min_score) return fail(c, VDET_EINVAL, "thresh and min_score must not be NaN");
    if (!d_score0_out) return fail(c, VDET_EINVAL, "null buffer");
    Videos vs;
    SoftNmsArgs a{};
    const int rc = tracknms_args(c, h_frame_off, V, C, T, d_tracks, d_ntracks, d_score, score_f64, d_tboxes, d_boxes, d_scores, B,
                                 d_keep_idx, d_keep_cnt, cap, top_still, thresh, R, d_tracks_out, d_score_out, d_src_out, d_cnt_out,
                                 d_ntracks_out, vs, a.tn);
    if (rc) return rc;
    a.oscore0 = d_score0_out; a.method = method; a.sigma32 = (float)sigma; a.min32 = (float)min_score;
    return tracknms_launch(c, a, a.tn, vs, softnms_kernel, kSnBytesPerCand);
}

int vdet_soft_nms_tracks(vdet_ctx *c, int64_t F, int64_t C, int T, const float *d_tracks, const int32_t *d_ntracks,
                         const void *d_score, int score_f64, const float *d_tboxes, const float *d_boxes, const float *d_scores,
                         int64_t B, const int32_t *d_keep_idx, const int32_t *d_keep_cnt, int64_t cap, int top_still, double thresh,
                         int R, int method, double sigma, double min_score, float *d_tracks_out, double *d_score_out,
                         int32_t *d_src_out, int32_t *d_cnt_out, int32_t *d_ntracks_out, double *d_score0_out)
{
    const int64_t off[2] = {0, F};
    return vdet_soft_nms_tracks_batch(c, off, 1, C, T, d_tracks, d_ntracks, d_score, score_f64, d_tboxes, d_boxes, d_scores, B,
                                      d_keep_idx, d_keep_cnt, cap, top_still, thresh, R, method, sigma, min_score, d_tracks_out,
                                      d_score_out, d_src_out, d_cnt_out, d_ntracks_out, d_score0_out);
}

// ---------------------------------------------------------------------------------------------
// Box voting on the same lists (votenms_kernels.hpp)
// ---------------------------------------------------------------------------------------------
int vdet_vote_nms_tracks_batch(vdet_ctx *c, const int64_t *h_frame_off, int64_t V, int64_t C, int T, const float *d_tracks,
                               const int32_t *d_ntracks, const void *d_score, int score_f64, const float *d_tboxes,
                               const float *d_boxes, const float *d_scores, int64_t B, const int32_t *d_keep_idx,
                               const int32_t *d_keep_cnt, int64_t cap, int top_still, double thresh, int R, double vote_thresh,
                               int weights, float *d_tracks_out, double *d_score_out, int32_t *d_src_out, int32_t *d_cnt_out,
                               int32_t *d_ntracks_out, float *d_box0_out, int32_t *d_votes_out)
{
    if (!c) return VDET_EINVAL;
    if (weights != kVnScore && weights != kVnUniform) return fail(c, VDET_EINVAL, "weights = %d; 0 (score) or 1 (uniform)", weights);
    if (vote_thresh != vote_thresh) return fail(c, VDET_EINVAL, "vote_thresh must not be NaN");
    if (!d_box0_out || !d_votes_out) return fail(c, VDET_EINVAL, "null buffer");
    Videos vs;
    VoteNmsArgs a{};
    const int rc = tracknms_args(c, h_frame_off, V, C, T, d_tracks, d_ntracks, d_score, score_f64, d_tboxes, d_boxes, d_scores, B,
                                 d_keep_idx, d_keep_cnt, cap, top_still, thresh, R, d_tracks_out, d_score_out, d_src_out, d_cnt_out,
                                 d_ntracks_out, vs, a.tn);
    if (rc) return rc;
    a.obox0 = d_box0_out; a.ovotes = d_votes_out; a.weights = weights; a.v32 = thresh_to_f32(vote_thresh);
    return tracknms_launch(c, a, a.tn, vs, votenms_kernel, kVnBytesPerCand);
}

int vdet_vote_nms_tracks(vdet_ctx *c, int64_t F, int64_t C, int T, const float *d_tracks, const int32_t *d_ntracks,
                         const void *d_score, int score_f64, const float *d_tboxes, const float *d_boxes, const float *d_scores,
                         int64_t B, const int32_t *d_keep_idx, const int32_t *d_keep_cnt, int64_t cap, int top_still, double thresh,
                         int R, double vote_thresh, int weights, float *d_tracks_out, double *d_score_out, int32_t *d_src_out,
                         int32_t *d_cnt_out, int32_t *d_ntracks_out, float *d_box0_out, int32_t *d_votes_out)
{
    const int64_t off[2] = {0, F};
    return vdet_vote_nms_tracks_batch(c, off, 1, C, T, d_tracks, d_ntracks, d_score, score_f64, d_tboxes, d_boxes, d_scores, B,
                                      d_keep_idx, d_keep_cnt, cap, top_still, thresh, R, vote_thresh, weights, d_tracks_out,
                                      d_score_out, d_src_out, d_cnt_out, d_ntracks_out, d_box0_out, d_votes_out);
}

// ---------------------------------------------------------------------------------------------
// Re-scoring of any tubelet set against the detections (rescore_kernels.hpp)
// ---------------------------------------------------------------------------------------------
int vdet_rescore_tubelets_batch(vdet_ctx *c, const int64_t *h_frame_off, int64_t V, int64_t B, int64_t C, int T, const float *d_tracks,
                                const int32_t *d_ntracks, const float *d_boxes, const float *d_scores, const void *d_floor,
                                int floor_f64, double overlap_thres, int complete, int window, double *d_det, double *d_pooled,
                                float *d_tboxes, int32_t *d_src)
{
    if (!c) return VDET_EINVAL;
    if (B <= 0 || C <= 0 || T < 0) return fail(c, VDET_EINVAL, "bad shape");
    if (window < 1 || window % 2 != 1) return fail(c, VDET_EINVAL, "Window size must be odd!");
    if (B > 32767) return fail(c, VDET_EINVAL, "B = %lld boxes per frame; the limit is 32767", (long long)B);
    Videos vs;
    int rc = read_videos(c, h_frame_off, V, 65535, &vs);
    if (rc) return rc;
    const int64_t F = vs.F, Fmax = vs.Fmax;
    if (!fits_upto(0x7FFFFFF0ll, {F, B}) || !fits_below(0x7FFFFFF0ll, {C, std::max(T, 1), F}) || !fits_below(0x7FFFFFF0ll, {V, C}))
        return fail(c, VDET_EINVAL, "volume too large (F*B and C*T*F must stay below 2^31 - 16)");
    if (T == 0) return VDET_OK;
    if (!d_tracks || !d_ntracks || !d_boxes || !d_scores || !d_det || !d_pooled || !d_tboxes || !d_src) return fail(c, VDET_EINVAL, "null buffer");
    if (((uintptr_t)d_boxes & 15) != 0) return fail(c, VDET_EINVAL, "d_boxes must be 16-byte aligned");
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    RescoreArgs g{};
    if (!c->no_index && !c->force_general && (size_t)8 * B + 24 * 1024 <= c->max_lds) {   // (the x1 sort must fit the LDS)
        // per-frame regular flags + x-sorted index over the concatenated volume: those of the graph build of the same boxes
        // when the cache holds them, else rebuilt here (as vdet_rescore_tracks does)
        if (!index_matches(c, d_boxes, F, B)) {
            c->graph_valid = c->lists_valid = c->index_valid = false;       // gflags / the index are rewritten
            if ((rc = volume_groups(c, F, B))) return rc;
            HIPCHK(c, c->gflags.reserve((size_t)F * 4));
            c->sym_built = false;
            hipLaunchKernelGGL(frame_flags_kernel, dim3((unsigned)F), dim3(256), 0, c->stream,
                               reinterpret_cast<const float4 *>(d_boxes), c->groups.as<GroupDesc>(), c->gflags.as<uint32_t>(),
                               &c->d_cnt->irregular);
            if ((rc = build_frame_index(c, reinterpret_cast<const float4 *>(d_boxes), F * B, F, (int)B))) return rc;
        }
        g.ix = frame_index_of(c);
        g.group_flags = c->gflags.as<uint32_t>();
    }
    if ((rc = video_table(c, c->anchor_tab, vs, &g.vids))) return rc;
    g.tracks = d_tracks; g.ntracks = d_ntracks; g.boxes = reinterpret_cast<const float4 *>(d_boxes); g.scores = d_scores;
    g.floor = d_floor; g.floor_f64 = floor_f64 ? 1 : 0;
    g.F = (int)F; g.B = (int)B; g.C = (int)C; g.T = T;
    g.thres = overlap_thres; g.complete = complete ? 1 : 0; g.window = window;
    g.det = d_det; g.pooled = d_pooled; g.tboxes = d_tboxes; g.src = d_src;
    g.err = &c->d_cnt->eindex;
    {
        StageTimer tm(c, ST_RSPATIAL);
        hipLaunchKernelGGL(rescore_tubelets_spatial_kernel, dim3((unsigned)((Fmax * C * T + 3) / 4), (unsigned)V), dim3(256), 0, c->stream, g);
    }
    {
        StageTimer tm(c, ST_RSERIES);
        // one wave per series with its present boxes in LDS, sized from the call's longest video; as many waves per workgroup
        // (4, 2, 1) as 64 KiB hold.  Videos too long for the stage take the one-thread-per-series kernel
        const int cap = (int)std::min<int64_t>(Fmax, kRescoreWaveMaxF);
        const int stride = (int)(((size_t)cap * kRescoreBytesPerFrame + 15) & ~(size_t)15);
        int waves = 4;
        while (waves > 1 && (size_t)waves * stride > 65536) waves >>= 1;
        hipLaunchKernelGGL(rescore_tubelets_series_kernel, dim3((unsigned)((C * T + waves - 1) / waves), (unsigned)V), dim3(64 * waves),
                           (size_t)waves * stride, c->stream, g, stride, cap);
        if (Fmax > cap)
            hipLaunchKernelGGL(rescore_tubelets_series_long_kernel, dim3((unsigned)((C * T + 63) / 64), (unsigned)V), dim3(64), 0, c->stream, g, cap);
    }
    HIPCHK(c, hipGetLastError());
    return VDET_OK;
}

int vdet_rescore_tubelets(vdet_ctx *c, int64_t F, int64_t B, int64_t C, int T, const float *d_tracks, const int32_t *d_ntracks,
                          const float *d_boxes, const float *d_scores, const void *d_floor, int floor_f64, double overlap_thres,
                          int complete, int window, double *d_det, double *d_pooled, float *d_tboxes, int32_t *d_src)
{
    const int64_t off[2] = {0, F};
    return vdet_rescore_tubelets_batch(c, off, 1, B, C, T, d_tracks, d_ntracks, d_boxes, d_scores, d_floor, floor_f64, overlap_thres,
                                       complete, window, d_det, d_pooled, d_tboxes, d_src);
}

// ---------------------------------------------------------------------------------------------
// R-CNN windows for the CNN scorers (patch_kernels.hpp)
// ---------------------------------------------------------------------------------------------
extern "C++" {
namespace {

int patch_check(vdet_ctx *c, const uint8_t *d_images, int64_t Fi, int64_t H, int64_t W, int S, int padding, int mode, int out_dtype,
                int64_t M, const void *d_patches)
{
    if (S < 1 || S > kPatchMaxS) return fail(c, VDET_EINVAL, "crop_size = %d; 1 .. %d", S, kPatchMaxS);
    if (padding < 0 || S - 2 * padding < 1) return fail(c, VDET_EINVAL, "padding = %d; 0 <= padding and crop_size - 2*padding >= 1", padding);
    if (mode != VDET_PATCH_WARP && mode != VDET_PATCH_SQUARE) return fail(c, VDET_EINVAL, "mode must be VDET_PATCH_WARP or VDET_PATCH_SQUARE");
    if (out_dtype != VDET_PATCH_F32 && out_dtype != VDET_PATCH_F16 && out_dtype != VDET_PATCH_BF16)
        return fail(c, VDET_EINVAL, "out_dtype must be VDET_PATCH_F32, VDET_PATCH_F16 or VDET_PATCH_BF16");
    if (Fi < 1 || H < 1 || W < 1 || H > kPatchMaxHW || W > kPatchMaxHW || Fi > 0x7FFFFFF0ll)
        return fail(c, VDET_EINVAL, "images must be [Fi,H,W,3] with Fi >= 1 and 1 <= H, W <= %d", kPatchMaxHW);
    if (M < 0 || M >= 0x7FFFFFF0ll) return fail(c, VDET_EINVAL, "too many windows (below 2^31 - 16)");
    if (M && (!d_images || !d_patches)) return fail(c, VDET_EINVAL, "null buffer");
    if (((uintptr_t)d_patches & 15) != 0) return fail(c, VDET_EINVAL, "d_patches must be 16-byte aligned");
    return VDET_OK;
}

template <typename OutT> void patch_launch_t(vdet_ctx *c, const PatchArgs &g, int vec, unsigned blocks)
{
    if (vec == 8) hipLaunchKernelGGL((rcnn_patches_kernel<OutT, 8>), dim3(blocks), dim3(256), 0, c->stream, g);
    else if (vec == 4) hipLaunchKernelGGL((rcnn_patches_kernel<OutT, 4>), dim3(blocks), dim3(256), 0, c->stream, g);
    else hipLaunchKernelGGL((rcnn_patches_kernel<OutT, 1>), dim3(blocks), dim3(256), 0, c->stream, g);
}

// one wave per (window, strip of kPatchRows rows), four per workgroup, on a 1-D grid
int patch_launch(vdet_ctx *c, PatchArgs &g, int out_dtype)
{
    if (g.M == 0) return VDET_OK;
    g.nstrips = (g.S + kPatchRows - 1) / kPatchRows;
    const int64_t blocks = (g.M * g.nstrips + 3) / 4;
    if (blocks > 0x7FFFFFFFll) return fail(c, VDET_EINVAL, "too many windows for one launch (windows * ceil(crop_size / %d) must stay below 2^33)", kPatchRows);
    const int vec16 = g.S % 8 == 0 ? 8 : g.S % 4 == 0 ? 4 : 1, vec32 = g.S % 4 == 0 ? 4 : 1;
    StageTimer tm(c, ST_OTHER);
    if (out_dtype == VDET_PATCH_F32) patch_launch_t<float>(c, g, vec32, (unsigned)blocks);
    else if (out_dtype == VDET_PATCH_F16) patch_launch_t<_Float16>(c, g, vec16, (unsigned)blocks);
    else patch_launch_t<PatchBf16>(c, g, vec16, (unsigned)blocks);
    return VDET_OK;
}

}  // namespace
}  // extern "C++"

int vdet_rcnn_patches(vdet_ctx *c, const uint8_t *d_images, int64_t Fi, int64_t H, int64_t W, const void *d_boxes, int boxes_f64,
                      int64_t N, const int32_t *d_image_idx, const double *d_offsets, int num, const double *d_mean, int S,
                      int padding, int mode, int out_dtype, void *d_patches, uint8_t *d_ok, double *d_sboxes)
{
    if (!c) return VDET_EINVAL;
    if (N < 0) return fail(c, VDET_EINVAL, "bad shape");
    if (num < 0 || num > kPatchMaxNum) return fail(c, VDET_EINVAL, "num = %d sampled boxes per box; 0 .. %d", num, kPatchMaxNum);
    if (!d_offsets) num = 0;
    const int64_t M = N * (num + 1);
    int rc = patch_check(c, d_images, Fi, H, W, S, padding, mode, out_dtype, M, d_patches);
    if (rc) return rc;
    if (M == 0) return VDET_OK;
    if (!d_boxes || !d_ok) return fail(c, VDET_EINVAL, "null buffer");
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    PatchArgs g{};
    g.images = d_images; g.Fi = (int)Fi; g.H = (int)H; g.W = (int)W;
    g.boxes = d_boxes; g.boxes_f64 = boxes_f64 ? 1 : 0; g.ld = 4;
    g.image_idx = d_image_idx; g.offsets = d_offsets; g.num = num;
    g.mean = d_mean; g.S = S; g.padding = padding; g.square = mode == VDET_PATCH_SQUARE ? 1 : 0;
    g.M = M; g.patches = d_patches; g.ok = d_ok; g.sboxes = d_sboxes;
    if ((rc = patch_launch(c, g, out_dtype))) return rc;
    HIPCHK(c, hipGetLastError());
    return VDET_OK;
}

int vdet_tubelet_patches(vdet_ctx *c, const uint8_t *d_images, int64_t Fi, int64_t H, int64_t W, const void *d_tracks, int tracks_f64,
                         int64_t C, int T, int64_t F, int ld, const int32_t *d_ntracks, int64_t f0, int64_t f1, int64_t cap,
                         const double *d_mean, int S, int padding, int mode, int out_dtype, void *d_patches, uint8_t *d_ok,
                         int32_t *d_slot, int32_t *d_count)
{
    if (!c) return VDET_EINVAL;
    if (C < 1 || T < 0 || F < 1 || ld < 4) return fail(c, VDET_EINVAL, "bad shape (tracks must be [C,T,F,>=4])");
    if (f0 < 0 || f1 <= f0 || f1 > F) return fail(c, VDET_EINVAL, "frames must be a range 0 <= f0 < f1 <= F");
    if (Fi != f1 - f0) return fail(c, VDET_EINVAL, "images must hold the f1 - f0 = %lld frames of the range", (long long)(f1 - f0));
    if (!fits_below(0x7FFFFFF0ll, {C, std::max(T, 1), F})) return fail(c, VDET_EINVAL, "too many tubelet boxes (C*T*F must stay below 2^31 - 16)");
    if (cap < 0) return fail(c, VDET_EINVAL, "cap must not be negative");
    int rc = patch_check(c, d_images, Fi, H, W, S, padding, mode, out_dtype, cap, d_patches);
    if (rc) return rc;
    if (!d_ntracks || !d_count || (T && !d_tracks) || (cap && (!d_slot || !d_ok))) return fail(c, VDET_EINVAL, "null buffer");
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    {
        StageTimer tm(c, ST_OTHER);
        hipLaunchKernelGGL(tubelet_slots_kernel, dim3(1), dim3(1024), 0, c->stream, d_tracks, tracks_f64 ? 1 : 0, ld, d_ntracks, (int)C, T,
                           F, f0, f1, cap, d_slot, d_count, &c->d_cnt->status);
    }
    PatchArgs g{};
    g.images = d_images; g.Fi = (int)Fi; g.H = (int)H; g.W = (int)W;
    g.boxes = d_tracks; g.boxes_f64 = tracks_f64 ? 1 : 0; g.ld = ld;
    g.slot = d_slot; g.T = T; g.F = F; g.f0 = f0;
    g.mean = d_mean; g.S = S; g.padding = padding; g.square = mode == VDET_PATCH_SQUARE ? 1 : 0;
    g.M = cap; g.patches = d_patches; g.ok = d_ok;
    if ((rc = patch_launch(c, g, out_dtype))) return rc;
    HIPCHK(c, hipGetLastError());
    return VDET_OK;
}

// ---------------------------------------------------------------------------------------------
// RoI pooling: the Fast R-CNN route (roipool_kernels.hpp)
// ---------------------------------------------------------------------------------------------
extern "C++" {
namespace {

int roi_check(vdet_ctx *c, const void *d_features, int feat_dtype, int64_t Fi, int64_t K, int64_t Hf, int64_t Wf, double spatial_scale,
              int ph, int pw, double box_scale, int mode, int sampling, int64_t N, const void *d_pooled)
{
    if (feat_dtype != VDET_FEAT_F32 && feat_dtype != VDET_FEAT_F16 && feat_dtype != VDET_FEAT_BF16)
        return fail(c, VDET_EINVAL, "feat_dtype must be VDET_FEAT_F32, VDET_FEAT_F16 or VDET_FEAT_BF16");
    if (Fi < 1 || K < 1 || Hf < 1 || Wf < 1 || Hf > kRoiMaxHW || Wf > kRoiMaxHW || Fi > 0x7FFFFFF0ll || K > 0x7FFFFFF0ll)
        return fail(c, VDET_EINVAL, "features must be [Fi,K,Hf,Wf] with Fi, K >= 1 and 1 <= Hf, Wf <= %d", kRoiMaxHW);
    if (ph < 1 || pw < 1 || ph > kRoiMaxPooled || pw > kRoiMaxPooled) return fail(c, VDET_EINVAL, "pooled = (%d, %d); 1 .. %d each", ph, pw, kRoiMaxPooled);
    if (mode != VDET_ROI_MAX && mode != VDET_ROI_ALIGN) return fail(c, VDET_EINVAL, "mode must be VDET_ROI_MAX or VDET_ROI_ALIGN");
    if (mode == VDET_ROI_ALIGN && (sampling < 1 || sampling > kRoiMaxSampling)) return fail(c, VDET_EINVAL, "sampling = %d; 1 .. %d", sampling, kRoiMaxSampling);
    if (!(spatial_scale > 0.0) || !(spatial_scale - spatial_scale == 0.0) || !((float)spatial_scale > 0.f) || !(box_scale - box_scale == 0.0))
        return fail(c, VDET_EINVAL, "spatial_scale must be positive and finite (also as float32), box_scale finite");
    if (N < 0 || N >= 0x7FFFFFF0ll) return fail(c, VDET_EINVAL, "too many RoIs (below 2^31 - 16)");
    if (N && (!d_features || !d_pooled)) return fail(c, VDET_EINVAL, "null buffer");
    return VDET_OK;
}

template <typename FeatT> void roi_launch_t(vdet_ctx *c, const RoiArgs &g, bool align, bool wpc, unsigned blocks)
{
    if (align && wpc) hipLaunchKernelGGL((roi_pool_kernel<FeatT, true, true>), dim3(blocks), dim3(256), 0, c->stream, g);
    else if (align) hipLaunchKernelGGL((roi_pool_kernel<FeatT, true, false>), dim3(blocks), dim3(256), 0, c->stream, g);
    else if (wpc) hipLaunchKernelGGL((roi_pool_kernel<FeatT, false, true>), dim3(blocks), dim3(256), 0, c->stream, g);
    else hipLaunchKernelGGL((roi_pool_kernel<FeatT, false, false>), dim3(blocks), dim3(256), 0, c->stream, g);
}

// the order of a workgroup's elements (roipool_kernels.hpp), by measurement: 'max' a wave per channel, 'align'
// lanes over the span.  VDET_ROIPOOL_ORDER = 1 / 2 forces span / wave per channel, for re-measuring
#ifndef VDET_ROIPOOL_ORDER
#define VDET_ROIPOOL_ORDER 0
#endif
bool roi_wave_per_channel(int mode) { return VDET_ROIPOOL_ORDER == 2 || (VDET_ROIPOOL_ORDER == 0 && mode == VDET_ROI_MAX); }

// one workgroup per (RoI, chunk of its output span), on a 1-D grid
int roi_launch(vdet_ctx *c, RoiArgs &g, int feat_dtype, int mode)
{
    if (g.N == 0) return VDET_OK;
    g.span = g.K * g.ph * g.pw;
    const bool wpc = roi_wave_per_channel(mode), align = mode == VDET_ROI_ALIGN;
    const int64_t nchunks = wpc ? (g.K + kRoiWaveCh - 1) / kRoiWaveCh : (g.span + kRoiChunk - 1) / kRoiChunk;
    if (!fits_upto(0x7FFFFFFFll, {g.N, nchunks})) return fail(c, VDET_EINVAL, "too many RoIs for one launch (N * ceil(K*ph*pw / %d) and N * ceil(K / %d) must stay below 2^31)", kRoiChunk, kRoiWaveCh);
    g.nchunks = (int)nchunks;
    const unsigned blocks = (unsigned)(g.N * nchunks);
    StageTimer tm(c, ST_OTHER);
    if (feat_dtype == VDET_FEAT_F32) roi_launch_t<float>(c, g, align, wpc, blocks);
    else if (feat_dtype == VDET_FEAT_F16) roi_launch_t<_Float16>(c, g, align, wpc, blocks);
    else roi_launch_t<PatchBf16>(c, g, align, wpc, blocks);
    return VDET_OK;
}

void roi_fill(RoiArgs &g, const void *d_features, int64_t Fi, int64_t K, int64_t Hf, int64_t Wf, double spatial_scale, int ph, int pw,
              double box_scale, int sampling, int aligned, void *d_pooled, uint8_t *d_ok)
{
    g.features = d_features; g.Fi = (int)Fi; g.K = K; g.Hf = (int)Hf; g.Wf = (int)Wf;
    g.spatial_scale = (float)spatial_scale; g.box_scale = box_scale;
    g.ph = ph; g.pw = pw; g.sampling = sampling; g.aligned = aligned ? 1 : 0;
    g.pooled = d_pooled; g.ok = d_ok;
}

}  // namespace
}  // extern "C++"

int vdet_roi_pool(vdet_ctx *c, const void *d_features, int feat_dtype, int64_t Fi, int64_t K, int64_t Hf, int64_t Wf, const void *d_boxes,
                  int boxes_f64, int64_t N, const int32_t *d_image_idx, double spatial_scale, int ph, int pw, double box_scale, int mode,
                  int sampling, int aligned, void *d_pooled, uint8_t *d_ok)
{
    if (!c) return VDET_EINVAL;
    int rc = roi_check(c, d_features, feat_dtype, Fi, K, Hf, Wf, spatial_scale, ph, pw, box_scale, mode, sampling, N, d_pooled);
    if (rc) return rc;
    if (N == 0) return VDET_OK;
    if (!d_boxes || !d_ok) return fail(c, VDET_EINVAL, "null buffer");
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    RoiArgs g{};
    roi_fill(g, d_features, Fi, K, Hf, Wf, spatial_scale, ph, pw, box_scale, sampling, aligned, d_pooled, d_ok);
    g.boxes = d_boxes; g.boxes_f64 = boxes_f64 ? 1 : 0; g.ld = 4;
    g.image_idx = d_image_idx; g.N = N;
    if ((rc = roi_launch(c, g, feat_dtype, mode))) return rc;
    HIPCHK(c, hipGetLastError());
    return VDET_OK;
}

int vdet_tubelet_rois(vdet_ctx *c, const void *d_features, int feat_dtype, int64_t Fi, int64_t K, int64_t Hf, int64_t Wf,
                      const void *d_tracks, int tracks_f64, int64_t C, int T, int64_t F, int ld, const int32_t *d_ntracks, int64_t f0,
                      int64_t f1, int64_t cap, double spatial_scale, int ph, int pw, double box_scale, int mode, int sampling, int aligned,
                      void *d_pooled, uint8_t *d_ok, int32_t *d_slot, int32_t *d_count)
{
    if (!c) return VDET_EINVAL;
    if (C < 1 || T < 0 || F < 1 || ld < 4) return fail(c, VDET_EINVAL, "bad shape (tracks must be [C,T,F,>=4])");
    if (f0 < 0 || f1 <= f0 || f1 > F) return fail(c, VDET_EINVAL, "frames must be a range 0 <= f0 < f1 <= F");
    if (Fi != f1 - f0) return fail(c, VDET_EINVAL, "features must hold the f1 - f0 = %lld frames of the range", (long long)(f1 - f0));
    if (!fits_below(0x7FFFFFF0ll, {C, std::max(T, 1), F})) return fail(c, VDET_EINVAL, "too many tubelet boxes (C*T*F must stay below 2^31 - 16)");
    if (cap < 0) return fail(c, VDET_EINVAL, "cap must not be negative");
    int rc = roi_check(c, d_features, feat_dtype, Fi, K, Hf, Wf, spatial_scale, ph, pw, box_scale, mode, sampling, cap, d_pooled);
    if (rc) return rc;
    if (!d_ntracks || !d_count || (T && !d_tracks) || (cap && (!d_slot || !d_ok))) return fail(c, VDET_EINVAL, "null buffer");
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    {
        StageTimer tm(c, ST_OTHER);
        hipLaunchKernelGGL(tubelet_slots_kernel, dim3(1), dim3(1024), 0, c->stream, d_tracks, tracks_f64 ? 1 : 0, ld, d_ntracks, (int)C, T,
                           F, f0, f1, cap, d_slot, d_count, &c->d_cnt->status);
    }
    RoiArgs g{};
    roi_fill(g, d_features, Fi, K, Hf, Wf, spatial_scale, ph, pw, box_scale, sampling, aligned, d_pooled, d_ok);
    g.boxes = d_tracks; g.boxes_f64 = tracks_f64 ? 1 : 0; g.ld = ld;
    g.slot = d_slot; g.T = T; g.F = F; g.f0 = f0; g.N = cap;
    if ((rc = roi_launch(c, g, feat_dtype, mode))) return rc;
    HIPCHK(c, hipGetLastError());
    return VDET_OK;
}

// ---------------------------------------------------------------------------------------------
// The SVM head of the CNN scorers (svmhead_kernels.hpp) and svm_scores on device pointers
// ---------------------------------------------------------------------------------------------
extern "C++" {
namespace {

template <typename FeatT, typename CT> void svm_head_launch_t(vdet_ctx *c, const SvmHeadArgs &g, bool vec, unsigned blocks)
{
    if (vec && g.K <= kSvmRound) hipLaunchKernelGGL((svm_head_kernel<FeatT, CT, 1, true>), dim3(blocks), dim3(256), 0, c->stream, g);
    else if (vec && g.K <= kSvmRegRounds * kSvmRound) hipLaunchKernelGGL((svm_head_kernel<FeatT, CT, 2, true>), dim3(blocks), dim3(256), 0, c->stream, g);
    else if (vec) hipLaunchKernelGGL((svm_head_kernel<FeatT, CT, 0, true>), dim3(blocks), dim3(256), 0, c->stream, g);
    else hipLaunchKernelGGL((svm_head_kernel<FeatT, CT, 0, false>), dim3(blocks), dim3(256), 0, c->stream, g);
}

template <typename CT> void svm_head_launch(vdet_ctx *c, const SvmHeadArgs &g, int feat_dtype, bool vec, unsigned blocks)
{
    if (feat_dtype == VDET_FEAT_F32) svm_head_launch_t<float, CT>(c, g, vec, blocks);
    else if (feat_dtype == VDET_FEAT_F16) svm_head_launch_t<_Float16, CT>(c, g, vec, blocks);
    else svm_head_launch_t<SvmBf16, CT>(c, g, vec, blocks);
}

template <typename T>
int svm_scores_dev_impl(vdet_ctx *c, const T *d_feat, int64_t n, int64_t k, const T *d_W, const T *d_B, int64_t m, T *d_out)
{
    if (!c) return VDET_EINVAL;
    if (n < 0 || k < 0 || m < 0) return fail(c, VDET_EINVAL, "bad shape");
    if (n == 0 || m == 0) return VDET_OK;
    if ((k > 0 && (!d_feat || !d_W)) || !d_out) return fail(c, VDET_EINVAL, "null buffer");
    if (n * k > ((int64_t)1 << 34) || k * m > ((int64_t)1 << 34) || n * m > ((int64_t)1 << 34)) return fail(c, VDET_EINVAL, "matrix too large");
    if ((n + 63) / 64 > 65535) return fail(c, VDET_EINVAL, "at most 65535 * 64 rows in one call");
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    {
        StageTimer tm(c, ST_OTHER);
        hipLaunchKernelGGL(svm_scores_kernel<T>, dim3((unsigned)((m + 63) / 64), (unsigned)((n + 63) / 64)), dim3(256), 0, c->stream, d_feat,
                           d_W, d_B, n, k, m, d_out);
    }
    HIPCHK(c, hipGetLastError());
    return VDET_OK;
}

}  // namespace
}  // extern "C++"

int vdet_svm_scores_dev_f64(vdet_ctx *c, const double *d_feat, int64_t n, int64_t k, const double *d_W, const double *d_B, int64_t m,
                            double *d_out)
{
    return svm_scores_dev_impl<double>(c, d_feat, n, k, d_W, d_B, m, d_out);
}

int vdet_svm_scores_dev_f32(vdet_ctx *c, const float *d_feat, int64_t n, int64_t k, const float *d_W, const float *d_B, int64_t m,
                            float *d_out)
{
    return svm_scores_dev_impl<float>(c, d_feat, n, k, d_W, d_B, m, d_out);
}

int vdet_svm_head(vdet_ctx *c, const void *d_feat, int feat_dtype, int64_t N, int G, int64_t K, const void *d_W, int w_f64,
                  const void *d_B, int b_f64, int64_t M, double scale, int compute_f64, const int32_t *d_slot, const int32_t *d_count,
                  int64_t C, int T, int64_t F, const int32_t *d_cols, const double *d_sboxes, const uint8_t *d_ok, void *d_det,
                  int32_t *d_arg, double *d_tboxes, void *d_score, int32_t *d_arg_flat, int32_t *d_nbad)
{
    if (!c) return VDET_EINVAL;
    if (N < 0 || G < 1 || K < 1 || M < 1) return fail(c, VDET_EINVAL, "bad shape (N >= 0 groups of G >= 1 windows, K >= 1 features, M >= 1 columns)");
    if (feat_dtype != VDET_FEAT_F32 && feat_dtype != VDET_FEAT_F16 && feat_dtype != VDET_FEAT_BF16 && feat_dtype != VDET_FEAT_F64)
        return fail(c, VDET_EINVAL, "feat_dtype must be VDET_FEAT_F32, VDET_FEAT_F16, VDET_FEAT_BF16 or VDET_FEAT_F64");
    if (!compute_f64 && (feat_dtype == VDET_FEAT_F64 || w_f64 || (d_B && b_f64)))
        return fail(c, VDET_EINVAL, "the compute type is f32 only when features, W and B are at most f32");
    if (!d_W || !d_nbad || (N && (!d_feat || !d_score || !d_arg_flat))) return fail(c, VDET_EINVAL, "null buffer");
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    if (N == 0) {
        HIPCHK(c, hipMemsetAsync(d_nbad, 0, sizeof(int32_t), c->stream));
        return VDET_OK;
    }
    if (d_slot ? (C < 1 || T < 1 || F < 1 || !fits_below(0x7FFFFFF0ll, {C, T, F})) : (C != 1))
        return fail(c, VDET_EINVAL, "shape must be C, T, F >= 1 with C*T*F below 2^31 - 16 (without slot: C = 1)");
    if (!fits_upto(1ll << 40, {K, M}) || !fits_upto(1ll << 46, {N, G, K})) return fail(c, VDET_EINVAL, "matrix too large");
    const size_t csz = compute_f64 ? 8 : 4;
    const int gpw = G >= 32 ? 1 : (32 + G - 1) / G;
    const int64_t nwaves = (N + gpw - 1) / gpw, blocks = (nwaves + 3) / 4;
    if (blocks > 0x7FFFFFFFll) return fail(c, VDET_EINVAL, "too many groups for one launch");
    HIPCHK(c, c->svm_wt.reserve((size_t)(M * K) * csz));
    HIPCHK(c, c->svm_wavebad.reserve((size_t)nwaves * sizeof(int32_t)));
    StageTimer tm(c, ST_OTHER);
    {
        const dim3 grid((unsigned)((M + 31) / 32), (unsigned)((K + 31) / 32)), block(32, 8);
        if (grid.y > 65535u || grid.x > 0x7FFFFFFFu) return fail(c, VDET_EINVAL, "matrix too large");
        if (compute_f64 && w_f64) hipLaunchKernelGGL((svm_wt_kernel<double, double>), grid, block, 0, c->stream, static_cast<const double *>(d_W), K, M, c->svm_wt.as<double>());
        else if (compute_f64) hipLaunchKernelGGL((svm_wt_kernel<float, double>), grid, block, 0, c->stream, static_cast<const float *>(d_W), K, M, c->svm_wt.as<double>());
        else hipLaunchKernelGGL((svm_wt_kernel<float, float>), grid, block, 0, c->stream, static_cast<const float *>(d_W), K, M, c->svm_wt.as<float>());
    }
    SvmHeadArgs g{};
    g.feat = d_feat; g.N = N; g.K = K; g.M = M; g.G = G;
    g.wt = c->svm_wt.p; g.bias = d_B; g.bias_f64 = b_f64 ? 1 : 0; g.scale = scale;
    g.slot = d_slot; g.count = d_count; g.cols = d_cols; g.C = C; g.F = F; g.T = T;
    g.sboxes = d_sboxes; g.ok = d_ok;
    g.det = d_slot ? d_det : nullptr; g.arg = d_slot ? d_arg : nullptr; g.tboxes = d_tboxes;
    g.score = d_score; g.arg_flat = d_arg_flat; g.wavebad = c->svm_wavebad.as<int32_t>();
    g.gpw = gpw; g.nwaves = nwaves; g.status = &c->d_cnt->status;
    const bool vec = K % kSvmUnit == 0 && ((uintptr_t)d_feat & 15) == 0;
    if (feat_dtype == VDET_FEAT_F64) svm_head_launch_t<double, double>(c, g, vec, (unsigned)blocks);
    else if (compute_f64) svm_head_launch<double>(c, g, feat_dtype, vec, (unsigned)blocks);
    else svm_head_launch<float>(c, g, feat_dtype, vec, (unsigned)blocks);
    hipLaunchKernelGGL(svm_nbad_kernel, dim3(1), dim3(1024), 0, c->stream, c->svm_wavebad.as<int32_t>(), nwaves, d_nbad);
    HIPCHK(c, hipGetLastError());
    return VDET_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// Device pixel tracker (pixtrack_kernels.hpp), fixed scale and with the scale search (tests/pixtrack_spec.py)
// ---------------------------------------------------------------------------------------------
// box sampling (tests/pixtrack_spec.py): the largest entry of a frame's integral, 255 * H * W, must fit in 32 bits
static int pix_box_check(vdet_ctx *c, int64_t H, int64_t W)
{
    if (H * W > kPixBoxMaxArea) return fail(c, VDET_EINVAL, "box sampling: frames of at most 2^24 pixels (H * W)");
    return VDET_OK;
}

// the template update's settings (vdet_track_pixels_adaptive, vdet_track_volume_pixels_adaptive; tests/pixtrack_adapt_spec.py)
static int pix_adapt_check(vdet_ctx *c, int box, int update, double update_conf, double drift_conf)
{
    if (box != 0 && box != 1) return fail(c, VDET_EINVAL, "box = %d; 0 (images) or 1 (integral)", box);
    if (update < 0 || update > 256) return fail(c, VDET_EINVAL, "update = %d; 0 .. 256", update);
    if (!std::isfinite(update_conf) || !std::isfinite(drift_conf)) return fail(c, VDET_EINVAL, "update_conf and drift_conf must be finite");
    return VDET_OK;
}

// vdet_track_pixels (sc null), vdet_track_pixels_scaled and -- box: d_images is the integral uint32 [F,H+1,W+1], sc is given --
// vdet_track_pixels_box; ad given (with sc): vdet_track_pixels_adaptive.  The settings' checks are pix_settings_check's
static int track_pixels_impl(vdet_ctx *c, const uint8_t *d_images, int64_t F, int64_t H, int64_t W, const int32_t *d_anchor_frames,
                             const float *d_anchor_boxes, const float *d_anchor_scores, int64_t C, int T, int S, int R, double min_conf,
                             int max_frames, int step, const PixScaleArgs *sc, float *d_tracks, float *d_anchors, int32_t *d_ntracks,
                             bool box = false, const PixAdaptArgs *ad = nullptr)
{
    if (!c) return VDET_EINVAL;
    if (F <= 0 || H <= 0 || W <= 0 || C <= 0 || T < 0) return fail(c, VDET_EINVAL, "bad shape");
    if (pix_settings_check(c, H, W, S, R, min_conf, max_frames, step, sc)) return VDET_EINVAL;
    if (box && pix_box_check(c, H, W)) return VDET_EINVAL;
    if (!fits_below(0x7FFFFFF0ll, {C, std::max(T, 1), F}))
        return fail(c, VDET_EINVAL, "volume too large (C*T*F must stay below 2^31 - 16)");
    if (!d_images || !d_ntracks || (T && (!d_anchor_frames || !d_anchor_boxes || !d_tracks || !d_anchors))) return fail(c, VDET_EINVAL, "null buffer");
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    if (T == 0) {
        HIPCHK(c, hipMemsetAsync(d_ntracks, 0, (size_t)C * 4, c->stream));
        return VDET_OK;
    }
    PixTrackArgs a{};
    a.images = d_images;
    a.F = (int)F; a.H = (int)H; a.W = (int)W; a.C = (int)C; a.T = T;
    a.aframes = d_anchor_frames; a.aboxes = d_anchor_boxes; a.ascores = d_anchor_scores;
    a.S = S; a.R = R;
    a.min_conf = (float)min_conf;
    a.reach = chain_reach(max_frames, (int)F);
    a.step = step;
    a.tracks = d_tracks; a.anchors = d_anchors; a.ntracks = d_ntracks;
    a.status = &c->d_cnt->status;
    {
        StageTimer tm(c, ST_OTHER);
        if (ad && box) hipLaunchKernelGGL(track_pixels_adaptive_box_kernel, dim3((unsigned)(C * T), 2), dim3(kPixLT), 0, c->stream, a, *sc, *ad);
        else if (ad) hipLaunchKernelGGL(track_pixels_adaptive_kernel, dim3((unsigned)(C * T), 2), dim3(kPixLT), 0, c->stream, a, *sc, *ad);
        else if (box) hipLaunchKernelGGL(track_pixels_box_kernel, dim3((unsigned)(C * T), 2), dim3(kPixLT), 0, c->stream, a, *sc);
        else if (sc) hipLaunchKernelGGL(track_pixels_scaled_kernel, dim3((unsigned)(C * T), 2), dim3(kPixLT), 0, c->stream, a, *sc);
        else hipLaunchKernelGGL(track_pixels_kernel, dim3((unsigned)(C * T), 2), dim3(kPixLT), 0, c->stream, a);
    }
    HIPCHK(c, hipGetLastError());
    return VDET_OK;
}

extern "C" {

int vdet_track_pixels(vdet_ctx *c, const uint8_t *d_images, int64_t F, int64_t H, int64_t W, const int32_t *d_anchor_frames,
                      const float *d_anchor_boxes, const float *d_anchor_scores, int64_t C, int T, int S, int R, double min_conf,
                      int max_frames, int step, float *d_tracks, float *d_anchors, int32_t *d_ntracks)
{
    return track_pixels_impl(c, d_images, F, H, W, d_anchor_frames, d_anchor_boxes, d_anchor_scores, C, T, S, R, min_conf, max_frames,
                             step, nullptr, d_tracks, d_anchors, d_ntracks);
}

int vdet_track_pixels_scaled(vdet_ctx *c, const uint8_t *d_images, int64_t F, int64_t H, int64_t W, const int32_t *d_anchor_frames,
                             const float *d_anchor_boxes, const float *d_anchor_scores, int64_t C, int T, int S, int R, double min_conf,
                             int max_frames, int step, int scales, int scale_step, int scale_penalty, float *d_tracks,
                             float *d_anchors, int32_t *d_ntracks)
{
    const PixScaleArgs sc{scales, scale_step, scale_penalty};
    return track_pixels_impl(c, d_images, F, H, W, d_anchor_frames, d_anchor_boxes, d_anchor_scores, C, T, S, R, min_conf, max_frames,
                             step, &sc, d_tracks, d_anchors, d_ntracks);
}

int vdet_luma_integral(vdet_ctx *c, const uint8_t *d_images, int64_t F, int64_t H, int64_t W, uint32_t *d_integral)
{
    if (!c) return VDET_EINVAL;
    if (F <= 0 || H <= 0 || W <= 0) return fail(c, VDET_EINVAL, "bad shape");
    if (H > 32767 || W > 32767) return fail(c, VDET_EINVAL, "images of at most 32767 rows and columns");
    if (pix_box_check(c, H, W)) return VDET_EINVAL;
    const int64_t nbx = (W + kPixIntColLT) / kPixIntColLT;                   // blocks over the W + 1 columns of a frame's table
    // (F*H is formed only once F itself is known to be small)
    const int64_t row_blocks = F >= 0x7FFFFFF0ll ? F : (F * H + kPixIntRowWaves - 1) / kPixIntRowWaves;
    if (row_blocks >= 0x7FFFFFF0ll || !fits_below(0x7FFFFFF0ll, {F, nbx}))
        return fail(c, VDET_EINVAL, "video too large (F*H/4 and F*ceil((W+1)/128) must stay below 2^31 - 16)");
    if (!d_images || !d_integral) return fail(c, VDET_EINVAL, "null buffer");
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    {
        StageTimer tm(c, ST_OTHER);
        hipLaunchKernelGGL(luma_integral_rows_kernel, dim3((unsigned)row_blocks), dim3(kPixIntRowLT), 0, c->stream, d_images, F * H, (int)H,
                           (int)W, d_integral);
        hipLaunchKernelGGL(luma_integral_cols_kernel, dim3((unsigned)(F * nbx)), dim3(kPixIntColLT), 0, c->stream, d_integral, (int)H,
                           (int)W, (int)nbx);
    }
    HIPCHK(c, hipGetLastError());
    return VDET_OK;
}

int vdet_track_pixels_box(vdet_ctx *c, const uint32_t *d_integral, int64_t F, int64_t H, int64_t W, const int32_t *d_anchor_frames,
                          const float *d_anchor_boxes, const float *d_anchor_scores, int64_t C, int T, int S, int R, double min_conf,
                          int max_frames, int step, int scales, int scale_step, int scale_penalty, float *d_tracks, float *d_anchors,
                          int32_t *d_ntracks)
{
    const PixScaleArgs sc{scales, scale_step, scale_penalty};
    return track_pixels_impl(c, reinterpret_cast<const uint8_t *>(d_integral), F, H, W, d_anchor_frames, d_anchor_boxes, d_anchor_scores,
                             C, T, S, R, min_conf, max_frames, step, &sc, d_tracks, d_anchors, d_ntracks, true);
}

int vdet_track_pixels_adaptive(vdet_ctx *c, const void *d_planes, int box, int64_t F, int64_t H, int64_t W,
                               const int32_t *d_anchor_frames, const float *d_anchor_boxes, const float *d_anchor_scores, int64_t C,
                               int T, int S, int R, double min_conf, int max_frames, int step, int scales, int scale_step,
                               int scale_penalty, int update, double update_conf, double drift_conf, float *d_tracks,
                               float *d_anchors, int32_t *d_ntracks)
{
    if (!c) return VDET_EINVAL;
    if (pix_adapt_check(c, box, update, update_conf, drift_conf)) return VDET_EINVAL;
    const PixScaleArgs sc{scales, scale_step, scale_penalty};
    const PixAdaptArgs ad{update, (float)update_conf, (float)drift_conf};
    return track_pixels_impl(c, static_cast<const uint8_t *>(d_planes), F, H, W, d_anchor_frames, d_anchor_boxes, d_anchor_scores, C, T,
                             S, R, min_conf, max_frames, step, &sc, d_tracks, d_anchors, d_ntracks, box == 1, &ad);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// Greedy tubelet generation with the pixel tracker (tests/pixtrack_spec.py): the greedy volume trackers' front half
// (volume_lists .. greedy_args, shared with vdet_nms_track_volume) and pick / lazy lists / eager pass, with
// pixtrack_kernels.hpp's chains as the tracker.  Three launches per track, no host wait.
// ---------------------------------------------------------------------------------------------
// vdet_track_volume_pixels (sc null), vdet_track_volume_pixels_scaled and -- box: d_images is the integral uint32 [F,H+1,W+1], sc
// is given -- vdet_track_volume_pixels_box; ad given (with sc): vdet_track_volume_pixels_adaptive
static int track_volume_pixels_impl(vdet_ctx *c, const uint8_t *d_images, int64_t H, int64_t W, const float *d_boxes, const float *d_scores,
                                    int64_t F, int64_t B, int64_t C, double nms_thres, double thres, int max_tracks, int S, int R,
                                    double min_conf, int max_frames, int step, const PixScaleArgs *sc, float *d_tracks,
                                    float *d_anchors, int32_t *d_ntracks, bool box = false, const PixAdaptArgs *ad = nullptr)
{
    if (!c) return VDET_EINVAL;
    if (F <= 0 || B <= 0 || C <= 0 || max_tracks < 0 || H <= 0 || W <= 0) return fail(c, VDET_EINVAL, "bad shape");
    if (!d_images || !d_boxes || !d_scores || !d_ntracks || (max_tracks > 0 && (!d_tracks || !d_anchors)))
        return fail(c, VDET_EINVAL, "null buffer");
    int rc = check_volume(c, d_boxes, F, B, C);
    if (rc) return rc;
    if (pix_settings_check(c, H, W, S, R, min_conf, max_frames, step, sc)) return VDET_EINVAL;
    if (box && pix_box_check(c, H, W)) return VDET_EINVAL;
    if (!fits_below(0x7FFFFFF0ll, {C, std::max(max_tracks, 1), F}))
        return fail(c, VDET_EINVAL, "volume too large (C*max_tracks*F must stay below 2^31 - 16)");
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    if ((rc = volume_lists(c, d_boxes, d_scores, F, B, C, nms_thres, true))) return rc;
    const TrackWork w = track_work(c, B, 0.5, max_frames, (int)F);      // (no link: link_thres is not used)
    if ((rc = pick_scratch(c, F, C, C))) return rc;
    if ((rc = track_begin(c, C, max_tracks, d_ntracks)) || max_tracks == 0) return rc;
    const GreedyArgs g = greedy_args(c, w, d_boxes, d_scores, F, B, C, nms_thres, thres, max_tracks, d_tracks, d_anchors, d_ntracks);
    PixTrackArgs pa{};
    pa.images = d_images;
    pa.F = (int)F; pa.H = (int)H; pa.W = (int)W;
    pa.S = S; pa.R = R;
    pa.min_conf = (float)min_conf;
    pa.reach = w.reach; pa.step = step;
    {
        StageTimer tm(c, ST_TLOOP);
        for (int t = 0; t < max_tracks; ++t) {
            hipLaunchKernelGGL(track_pick_kernel, dim3((unsigned)C), dim3(256), 0, c->stream, g.la, g.lz, g.sp);
            if (ad && box) hipLaunchKernelGGL(track_pixel_chain_adaptive_box_kernel, dim3((unsigned)C, 2), dim3(kPixLT), 0, c->stream, pa,
                                              *sc, *ad, (const TrackState *)g.sp.st, d_boxes, (int)B, max_tracks, d_tracks,
                                              &c->d_cnt->status);
            else if (ad) hipLaunchKernelGGL(track_pixel_chain_adaptive_kernel, dim3((unsigned)C, 2), dim3(kPixLT), 0, c->stream, pa, *sc,
                                            *ad, (const TrackState *)g.sp.st, d_boxes, (int)B, max_tracks, d_tracks, &c->d_cnt->status);
            else if (box) hipLaunchKernelGGL(track_pixel_chain_box_kernel, dim3((unsigned)C, 2), dim3(kPixLT), 0, c->stream, pa, *sc,
                                        (const TrackState *)g.sp.st, d_boxes, (int)B, max_tracks, d_tracks, &c->d_cnt->status);
            else if (sc) hipLaunchKernelGGL(track_pixel_chain_scaled_kernel, dim3((unsigned)C, 2), dim3(kPixLT), 0, c->stream, pa, *sc,
                                       (const TrackState *)g.sp.st, d_boxes, (int)B, max_tracks, d_tracks, &c->d_cnt->status);
            else hipLaunchKernelGGL(track_pixel_chain_kernel, dim3((unsigned)C, 2), dim3(kPixLT), 0, c->stream, pa,
                                    (const TrackState *)g.sp.st, d_boxes, (int)B, max_tracks, d_tracks, &c->d_cnt->status);
            hipLaunchKernelGGL(track_suppress_commit_kernel, dim3((unsigned)C), dim3(256), (size_t)w.mask_words * 16, c->stream, g.la, g.sp);
        }
    }
    HIPCHK(c, hipGetLastError());
    return VDET_OK;
}

extern "C" {

int vdet_track_volume_pixels(vdet_ctx *c, const uint8_t *d_images, int64_t H, int64_t W, const float *d_boxes, const float *d_scores,
                             int64_t F, int64_t B, int64_t C, double nms_thres, double thres, int max_tracks, int S, int R,
                             double min_conf, int max_frames, int step, float *d_tracks, float *d_anchors, int32_t *d_ntracks)
{
    return track_volume_pixels_impl(c, d_images, H, W, d_boxes, d_scores, F, B, C, nms_thres, thres, max_tracks, S, R, min_conf,
                                    max_frames, step, nullptr, d_tracks, d_anchors, d_ntracks);
}

int vdet_track_volume_pixels_scaled(vdet_ctx *c, const uint8_t *d_images, int64_t H, int64_t W, const float *d_boxes,
                                    const float *d_scores, int64_t F, int64_t B, int64_t C, double nms_thres, double thres,
                                    int max_tracks, int S, int R, double min_conf, int max_frames, int step, int scales,
                                    int scale_step, int scale_penalty, float *d_tracks, float *d_anchors, int32_t *d_ntracks)
{
    const PixScaleArgs sc{scales, scale_step, scale_penalty};
    return track_volume_pixels_impl(c, d_images, H, W, d_boxes, d_scores, F, B, C, nms_thres, thres, max_tracks, S, R, min_conf,
                                    max_frames, step, &sc, d_tracks, d_anchors, d_ntracks);
}

int vdet_track_volume_pixels_box(vdet_ctx *c, const uint32_t *d_integral, int64_t H, int64_t W, const float *d_boxes,
                                 const float *d_scores, int64_t F, int64_t B, int64_t C, double nms_thres, double thres,
                                 int max_tracks, int S, int R, double min_conf, int max_frames, int step, int scales, int scale_step,
                                 int scale_penalty, float *d_tracks, float *d_anchors, int32_t *d_ntracks)
{
    const PixScaleArgs sc{scales, scale_step, scale_penalty};
    return track_volume_pixels_impl(c, reinterpret_cast<const uint8_t *>(d_integral), H, W, d_boxes, d_scores, F, B, C, nms_thres, thres,
                                    max_tracks, S, R, min_conf, max_frames, step, &sc, d_tracks, d_anchors, d_ntracks, true);
}

int vdet_track_volume_pixels_adaptive(vdet_ctx *c, const void *d_planes, int box, int64_t H, int64_t W, const float *d_boxes,
                                      const float *d_scores, int64_t F, int64_t B, int64_t C, double nms_thres, double thres,
                                      int max_tracks, int S, int R, double min_conf, int max_frames, int step, int scales,
                                      int scale_step, int scale_penalty, int update, double update_conf, double drift_conf,
                                      float *d_tracks, float *d_anchors, int32_t *d_ntracks)
{
    if (!c) return VDET_EINVAL;
    if (pix_adapt_check(c, box, update, update_conf, drift_conf)) return VDET_EINVAL;
    const PixScaleArgs sc{scales, scale_step, scale_penalty};
    const PixAdaptArgs ad{update, (float)update_conf, (float)drift_conf};
    return track_volume_pixels_impl(c, static_cast<const uint8_t *>(d_planes), H, W, d_boxes, d_scores, F, B, C, nms_thres, thres,
                                    max_tracks, S, R, min_conf, max_frames, step, &sc, d_tracks, d_anchors, d_ntracks, box == 1, &ad);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// Motion-guided propagation of detections (motion_kernels.hpp; the rule is tests/motion_spec.py): the block-motion field of
// every frame pair with its summed table, and the boxes of the keep lists moved along it.  No scratch, no host wait; nothing
// of the prep cache is read or written.
// ---------------------------------------------------------------------------------------------
namespace {

// the launch of motion_table_kernel, inside the caller's timed span
void motion_table_launch(vdet_ctx *c, const int16_t *d_field, int64_t F, int64_t Hb, int64_t Wb, int32_t *d_fsum)
{
    hipLaunchKernelGGL(motion_table_kernel, dim3((unsigned)(2 * F)), dim3(64), 0, c->stream, reinterpret_cast<const uint32_t *>(d_field),
                       (int)Hb, (int)Wb, reinterpret_cast<int2 *>(d_fsum));
}

// the shape of a field and its table: 1 .. 4096 block rows and columns, every element count below 2^31 - 16
int motion_table_check(vdet_ctx *c, int64_t F, int64_t Hb, int64_t Wb)
{
    if (F <= 0 || Hb <= 0 || Wb <= 0) return fail(c, VDET_EINVAL, "bad shape");
    if (Hb > kMoTabRows || Wb > kMoTabRows) return fail(c, VDET_EINVAL, "a motion field of at most %d block rows and columns", kMoTabRows);
    if (!fits_below(0x7FFFFFF0ll, {4, F, Hb + 1, Wb + 1}))
        return fail(c, VDET_EINVAL, "motion field too large (2*F*(Hb+1)*(Wb+1)*2 must stay below 2^31 - 16)");
    return VDET_OK;
}

}  // namespace

extern "C" {

int vdet_motion_table(vdet_ctx *c, const int16_t *d_field, int64_t F, int64_t Hb, int64_t Wb, int32_t *d_fsum)
{
    if (!c) return VDET_EINVAL;
    if (motion_table_check(c, F, Hb, Wb)) return VDET_EINVAL;
    if (!d_field || !d_fsum) return fail(c, VDET_EINVAL, "null buffer");
    if (((uintptr_t)d_field & 3) != 0 || ((uintptr_t)d_fsum & 7) != 0) return fail(c, VDET_EINVAL, "d_field must be 4-byte and d_fsum 8-byte aligned");
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    {
        StageTimer tm(c, ST_OTHER);
        motion_table_launch(c, d_field, F, Hb, Wb, d_fsum);
    }
    HIPCHK(c, hipGetLastError());
    return VDET_OK;
}

int vdet_motion_field(vdet_ctx *c, const uint8_t *d_images, int64_t F, int64_t H, int64_t W, int block, int radius, int16_t *d_field,
                      int32_t *d_cost, int32_t *d_fsum)
{
    if (!c) return VDET_EINVAL;
    if (F <= 0 || H <= 0 || W <= 0) return fail(c, VDET_EINVAL, "bad shape");
    if (H > 32767 || W > 32767) return fail(c, VDET_EINVAL, "images of at most 32767 rows and columns");
    if (block != 8 && block != 16 && block != 32) return fail(c, VDET_EINVAL, "block = %d; 8, 16 or 32", block);
    if (radius < 1 || radius > kMoMaxR) return fail(c, VDET_EINVAL, "radius = %d; 1 .. %d", radius, kMoMaxR);
    const int64_t Hb = (H + block - 1) / block, Wb = (W + block - 1) / block;
    if (motion_table_check(c, F, Hb, Wb)) return VDET_EINVAL;
    const int64_t ty = (H + kMoTile - 1) / kMoTile, tx = (W + kMoTile - 1) / kMoTile;
    if (!d_images || !d_field || !d_cost || !d_fsum) return fail(c, VDET_EINVAL, "null buffer");
    if (((uintptr_t)d_field & 3) != 0 || ((uintptr_t)d_fsum & 7) != 0) return fail(c, VDET_EINVAL, "d_field must be 4-byte and d_fsum 8-byte aligned");
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    MotionArgs a{};
    a.images = d_images;
    a.F = (int)F; a.H = (int)H; a.W = (int)W; a.R = radius;
    a.Hb = (int)Hb; a.Wb = (int)Wb; a.ty = (int)ty; a.tx = (int)tx;
    // lanes per block: the width that wastes the fewest lanes on (2R+1)^2 candidates, among those that divide the tile's
    // (64/block)^2 blocks evenly over the waves
    const int nblk = (kMoTile / block) * (kMoTile / block), ncand = (2 * radius + 1) * (2 * radius + 1);
    int best = 0;
    for (int gw = 64; gw >= 16; gw >>= 1) {
        if (nblk % (kMoWaves * 64 / gw)) continue;
        const int trips = (ncand + gw - 1) / gw * gw;
        if (!best || trips < (ncand + best - 1) / best * best) best = gw;
    }
    a.gw = best;
    a.field = reinterpret_cast<uint32_t *>(d_field);
    a.cost = d_cost;
    const dim3 grid((unsigned)(ty * tx * F * 2));            // (<= 2 * F * Hb * Wb: checked above)
    {
        StageTimer tm(c, ST_OTHER);
        if (block == 8) hipLaunchKernelGGL(motion_match_kernel<8>, grid, dim3(kMoLT), 0, c->stream, a);
        else if (block == 16) hipLaunchKernelGGL(motion_match_kernel<16>, grid, dim3(kMoLT), 0, c->stream, a);
        else hipLaunchKernelGGL(motion_match_kernel<32>, grid, dim3(kMoLT), 0, c->stream, a);
        motion_table_launch(c, d_field, F, Hb, Wb, d_fsum);
    }
    HIPCHK(c, hipGetLastError());
    return VDET_OK;
}

int vdet_propagate_boxes(vdet_ctx *c, const int32_t *d_fsum, int64_t F, int64_t Hb, int64_t Wb, int block, int64_t H, int64_t W,
                         int64_t B, int64_t C, const float *d_boxes, const float *d_scores, const int32_t *d_keep_idx, int64_t kcap,
                         const int32_t *d_keep_cnt, int top, int reach, double decay, float *d_tracks, float *d_score,
                         int32_t *d_src, int32_t *d_ntracks)
{
    if (!c) return VDET_EINVAL;
    if (F <= 0 || H <= 0 || W <= 0 || B <= 0 || C <= 0 || kcap <= 0) return fail(c, VDET_EINVAL, "bad shape");
    if (H > 32767 || W > 32767) return fail(c, VDET_EINVAL, "images of at most 32767 rows and columns");
    if (block != 8 && block != 16 && block != 32) return fail(c, VDET_EINVAL, "block = %d; 8, 16 or 32", block);
    if (Hb != (H + block - 1) / block || Wb != (W + block - 1) / block)
        return fail(c, VDET_EINVAL, "the table is not the one of %lld x %lld images in blocks of %d", (long long)H, (long long)W, block);
    if (motion_table_check(c, F, Hb, Wb)) return VDET_EINVAL;
    if (B > 32767) return fail(c, VDET_EINVAL, "B = %lld boxes per frame; the limit is 32767", (long long)B);
    if (top < 1 || top > kcap) return fail(c, VDET_EINVAL, "top = %d; 1 .. the capacity of the keep lists (%lld)", top, (long long)kcap);
    if (reach < 1 || reach > kMoMaxReach) return fail(c, VDET_EINVAL, "reach = %d; 1 .. %d", reach, kMoMaxReach);
    const int64_t T = 2 * (int64_t)reach * top;
    if (T > 1024) return fail(c, VDET_EINVAL, "2*reach*top = %lld slots per class; the limit is 1024", (long long)T);
    if (!(decay >= 0.0) || !std::isfinite(decay)) return fail(c, VDET_EINVAL, "decay must be finite and >= 0");
    if (!fits_below(0x7FFFFFF0ll, {C, T, F}) || kcap >= 0x7FFFFFF0ll)
        return fail(c, VDET_EINVAL, "volume too large (C*T*F must stay below 2^31 - 16)");
    if (!d_fsum || !d_boxes || !d_scores || !d_keep_idx || !d_keep_cnt || !d_tracks || !d_score || !d_src || !d_ntracks)
        return fail(c, VDET_EINVAL, "null buffer");
    if (((uintptr_t)d_fsum & 7) != 0) return fail(c, VDET_EINVAL, "d_fsum must be 8-byte aligned");
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    PropagateArgs a{};
    a.fsum = reinterpret_cast<const int2 *>(d_fsum);
    a.F = (int)F; a.Hb = (int)Hb; a.Wb = (int)Wb; a.P = block; a.H = (int)H; a.W = (int)W; a.B = (int)B; a.C = (int)C;
    a.boxes = d_boxes; a.scores = d_scores; a.keep_idx = d_keep_idx; a.keep_cnt = d_keep_cnt;
    a.kcap = (int)kcap; a.top = top; a.reach = reach;
    a.decay = (float)decay;
    a.tracks = d_tracks; a.score = d_score; a.src = d_src; a.ntracks = d_ntracks;
    a.status = &c->d_cnt->status;
    const int64_t threads = C * 2 * top * F;                 // (= C*T*F / reach)
    {
        StageTimer tm(c, ST_OTHER);
        hipLaunchKernelGGL(propagate_boxes_kernel, dim3((unsigned)((threads + kMoPropLT - 1) / kMoPropLT)), dim3(kMoPropLT), 0, c->stream, a);
    }
    HIPCHK(c, hipGetLastError());
    return VDET_OK;
}

// ---------------------------------------------------------------------------------------------
// Multi-context suppression (context_kernels.hpp)
// ---------------------------------------------------------------------------------------------
}  // extern "C"

namespace {

// records a video of `ne` elements may write (0: none, the full-read passes)
uint32_t ctxs_cap(const vdet_ctx *c, int64_t ne)
{
    if (!c->ctxs_records) return 0u;
    return (uint32_t)std::min<int64_t>(kCtxRecMax, std::max<int64_t>(kCtxRecMin, ne / 64));
}

// THE shape check and video table of both entry points: one video by value (*one, no host table), or the staged table of V
// videos keyed by the offsets and the shape.  *chunks: chunks of the longest video; *cap_max / *rec_total: the record slices.
int ctxs_videos(vdet_ctx *c, int64_t F, int64_t B, int64_t C, const int64_t *h_frame_off, int64_t V, CtxVid *one, int64_t *nv,
                int64_t *chunks, uint32_t *cap_max, int64_t *rec_total)
{
    if (F <= 0 || B <= 0 || C <= 0) return fail(c, VDET_EINVAL, "bad shape");
    if (!fits_upto(0x7FFFFFF0ll, {F, B})) return fail(c, VDET_EINVAL, "volume too large (F*B must stay below 2^31 - 16)");
    // the class of an element is (class of the chunk's first element + offset in the chunk) % C in 32-bit arithmetic: the sum
    // (< C + kCtxChunk + 4) and the suppress kernel's running class (< 2 C) must fit 32 bits.  No other limit on C.
    if (C > 0x7FFF0000ll) return fail(c, VDET_EINVAL, "C = %lld classes; the limit is 2^31 - 65536", (long long)C);
    Videos vs;
    const int rc = read_videos_or_one(c, h_frame_off, V, F, 65535, &vs);
    if (rc) return rc;
    const int64_t Fmax = vs.Fmax;
    *nv = vs.V;
    if (!fits_upto(0xFFFFFFFFll, {Fmax, B, C})) return fail(c, VDET_EINVAL, "a video of 2^32 scores or more (the counters are 32 bits wide)");
    *chunks = (Fmax * B * C + kCtxChunk - 1) / kCtxChunk;
    *cap_max = ctxs_cap(c, Fmax * B * C);
    if (!h_frame_off) {
        *one = CtxVid{0, F * B * C, 0, *cap_max, 0u};
        *rec_total = *cap_max;
        return VDET_OK;
    }
    int64_t total = 0;
    for (int64_t v = 0; v < V; ++v) total += ctxs_cap(c, (h_frame_off[v + 1] - h_frame_off[v]) * B * C);
    *rec_total = total;
    std::vector<int64_t> key(h_frame_off, h_frame_off + V + 1);
    key.push_back(B); key.push_back(C); key.push_back(c->ctxs_records ? 1 : 0);
    return stage_keyed(c, c->ctxs_tab, key.data(), key.size() * 8, (size_t)V * sizeof(CtxVid), [&](char *dst) {
        CtxVid *tab = reinterpret_cast<CtxVid *>(dst);
        int64_t rec0 = 0;
        for (int64_t v = 0; v < V; ++v) {
            const int64_t ne = (h_frame_off[v + 1] - h_frame_off[v]) * B * C;
            tab[v] = CtxVid{h_frame_off[v] * B * C, ne, rec0, ctxs_cap(c, ne), 0u};
            rec0 += tab[v].cap;
        }
    });
}

}  // namespace

extern "C" {

int vdet_context_classes(vdet_ctx *c, const float *d_scores, int64_t F, int64_t B, int64_t C, double ratio, int64_t top,
                         int64_t min_hits, int use_score_thresh, double score_thresh, const int64_t *h_frame_off, int64_t V,
                         float *d_thresh, int64_t *d_n, int32_t *d_hits, uint8_t *d_high)
{
    if (!c) return VDET_EINVAL;
    if (top < 0) return fail(c, VDET_EINVAL, "top must be at least 1 (0: by ratio)");
    if (top == 0 && !(ratio > 0.0 && ratio <= 1.0)) return fail(c, VDET_EINVAL, "ratio must lie in (0, 1]");
    if (min_hits < 1) return fail(c, VDET_EINVAL, "min_hits must be at least 1");
    if (!d_scores || !d_thresh || !d_n || !d_hits || !d_high) return fail(c, VDET_EINVAL, "null buffer");
    if (((uintptr_t)d_scores & 3) != 0) return fail(c, VDET_EINVAL, "d_scores must be 4-byte aligned");
    CtxArgs a{};
    int64_t nv = 1, chunks = 0, rec_total = 0;
    uint32_t cap_max = 0;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = ctxs_videos(c, F, B, C, h_frame_off, V, &a.one, &nv, &chunks, &cap_max, &rec_total);
    if (rc) return rc;
    timing_reset(c);
    HIPCHK(c, c->ctxs_hist.reserve((size_t)nv * kCtxBins * 4));
    HIPCHK(c, c->ctxs_state.reserve((size_t)nv * sizeof(CtxState)));
    HIPCHK(c, c->ctxs_rec.reserve(std::max<size_t>((size_t)rec_total * 8, 16)));
    HIPCHK(c, hipMemsetAsync(c->ctxs_hist.p, 0, (size_t)nv * kCtxBins * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(d_hits, 0, (size_t)(nv * C) * 4, c->stream));
    c->ctxs_last_videos = nv;
    a.scores = d_scores;
    a.vids = h_frame_off ? c->ctxs_tab.dev.as<CtxVid>() : nullptr;
    a.V = (int)nv; a.C = (int)C;
    a.use_thr = use_score_thresh ? 1 : 0; a.thr = (float)score_thresh;
    a.ratio = ratio; a.top = top; a.min_hits = min_hits;
    a.hist = c->ctxs_hist.as<uint32_t>(); a.state = c->ctxs_state.as<CtxState>(); a.rec = c->ctxs_rec.as<uint2>();
    a.othresh = d_thresh; a.on = d_n; a.ohits = d_hits; a.ohigh = d_high;
    const dim3 gvol((unsigned)chunks, (unsigned)nv), gsel((unsigned)nv);
    const dim3 grec((unsigned)((cap_max + 1023u) / 1024u), (unsigned)nv);
    {
        StageTimer tm(c, ST_TPICK);
        hipLaunchKernelGGL(ctxs_hist_kernel<0>, gvol, dim3(kCtxLT), 0, c->stream, a);
        hipLaunchKernelGGL(ctxs_select_kernel, gsel, dim3(256), 0, c->stream, a, 0);
        hipLaunchKernelGGL(ctxs_hist_kernel<1>, gvol, dim3(kCtxLT), 0, c->stream, a);
        hipLaunchKernelGGL(ctxs_select_kernel, gsel, dim3(256), 0, c->stream, a, 1);
        if (cap_max) hipLaunchKernelGGL(ctxs_rec_hist_kernel, grec, dim3(kCtxLT), 0, c->stream, a);
        hipLaunchKernelGGL(ctxs_hist_kernel<2>, gvol, dim3(kCtxLT), 0, c->stream, a);
        hipLaunchKernelGGL(ctxs_select_kernel, gsel, dim3(256), 0, c->stream, a, 2);
        if (cap_max) hipLaunchKernelGGL(ctxs_rec_hits_kernel, dim3((cap_max + kCtxHitsPer - 1) / kCtxHitsPer, (unsigned)nv), dim3(kCtxLT), 0, c->stream, a);
        hipLaunchKernelGGL(ctxs_hits_kernel, gvol, dim3(kCtxLT), 0, c->stream, a);
        hipLaunchKernelGGL(ctxs_finish_kernel, dim3((unsigned)((C + 255) / 256), (unsigned)nv), dim3(256), 0, c->stream, a);
    }
    HIPCHK(c, hipGetLastError());
    return VDET_OK;
}

int vdet_suppress_context(vdet_ctx *c, const float *d_scores, int64_t F, int64_t B, int64_t C, const uint8_t *d_high,
                          double penalty, const int64_t *h_frame_off, int64_t V, float *d_out)
{
    if (!c) return VDET_EINVAL;
    if (!std::isfinite(penalty) || penalty < 0.0 || !std::isfinite((float)penalty))
        return fail(c, VDET_EINVAL, "penalty must be finite (as a float32) and >= 0");
    if (!d_scores || !d_high || !d_out) return fail(c, VDET_EINVAL, "null buffer");
    if (((uintptr_t)d_scores & 3) != 0 || ((uintptr_t)d_out & 3) != 0) return fail(c, VDET_EINVAL, "d_scores and d_out must be 4-byte aligned");
    CtxSuppressArgs a{};
    int64_t nv = 1, chunks = 0, rec_total = 0;
    uint32_t cap_max = 0;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = ctxs_videos(c, F, B, C, h_frame_off, V, &a.one, &nv, &chunks, &cap_max, &rec_total);
    if (rc) return rc;
    if (d_out != d_scores) {
        const uintptr_t s0 = (uintptr_t)d_scores, o0 = (uintptr_t)d_out, bytes = (uintptr_t)(F * B * C) * 4;
        if (s0 < o0 + bytes && o0 < s0 + bytes) return fail(c, VDET_EINVAL, "d_out must be d_scores itself or not overlap it");
    }
    timing_reset(c);
    a.in = d_scores; a.out = d_out; a.high = d_high;
    a.vids = h_frame_off ? c->ctxs_tab.dev.as<CtxVid>() : nullptr;
    a.C = (int)C; a.penalty = (float)penalty;
    {
        StageTimer tm(c, ST_OTHER);
        hipLaunchKernelGGL(ctxs_suppress_kernel, dim3((unsigned)chunks, (unsigned)nv), dim3(kCtxLT), 0, c->stream, a);
    }
    HIPCHK(c, hipGetLastError());
    return VDET_OK;
}

// ---------------------------------------------------------------------------------------------
// Seq-NMS (seqnms_kernels.hpp)
// ---------------------------------------------------------------------------------------------
int vdet_seq_nms_batch(vdet_ctx *c, const int64_t *h_frame_off, int64_t V, int64_t C, int R, const float *d_tracks,
                       const int32_t *d_ntracks, const void *d_score, int score_f64, double link_thres, double nms_thres,
                       int rescore, int max_seqs, double min_score, float *d_tracks_out, double *d_score_out, int32_t *d_seq_out,
                       int32_t *d_ntracks_out, int32_t *d_nseq, double *d_seq_sum, int32_t *d_seq_len, int32_t *d_seq_end,
                       uint8_t *d_exhausted)
{
    if (!c) return VDET_EINVAL;
    if (C < 1) return fail(c, VDET_EINVAL, "bad shape");
    Videos vs;
    int rc = read_videos(c, h_frame_off, V, 65535, &vs);
    if (rc) return rc;
    const int64_t F = vs.F, Fmax = vs.Fmax;
    if (R < 1 || R > kSqMaxR) return fail(c, VDET_EINVAL, "R = %d rows per (frame, class); 1 .. %d (cut wider lists with vdet_nms_tracks' R)", R, kSqMaxR);
    if (max_seqs < 1 || max_seqs > kSqMaxSeqs) return fail(c, VDET_EINVAL, "max_seqs = %d; 1 .. %d", max_seqs, kSqMaxSeqs);
    if (rescore != 0 && rescore != 1) return fail(c, VDET_EINVAL, "rescore must be 0 (average) or 1 (maximum)");
    if (!std::isfinite(link_thres) || !std::isfinite(nms_thres)) return fail(c, VDET_EINVAL, "link_thres and nms_thres must be finite");
    if (min_score != min_score) return fail(c, VDET_EINVAL, "min_score must not be NaN");
    const int64_t W = (R + 31) / 32, Rp = (R + 63) / 64 * 64;
    if (!fits_below(0x7FFFFFF0ll, {C, R, F}))
        return fail(c, VDET_EINVAL, "too many boxes (C*R*F must stay below 2^31 - 16)");
    if (!fits_below(0x7FFFFFF0ll, {C, R, F, W}))
        return fail(c, VDET_EINVAL, "too many link words (C*F*R*ceil(R/32) must stay below 2^31 - 16)");
    if (!fits_below(0x7FFFFFF0ll, {C, V, max_seqs}))
        return fail(c, VDET_EINVAL, "too many sequences (C*max_seqs*V must stay below 2^31 - 16)");
    if (!d_tracks || !d_ntracks) return fail(c, VDET_EINVAL, "null buffer");
    if (!d_tracks_out || !d_score_out || !d_seq_out || !d_ntracks_out || !d_nseq || !d_seq_sum || !d_seq_len || !d_seq_end || !d_exhausted)
        return fail(c, VDET_EINVAL, "null buffer");
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    SeqNmsArgs g{};
    if ((rc = video_table(c, c->anchor_tab, vs, &g.vids))) return rc;
    // the predecessor table of the longest video: in LDS while it fits the budget (and the device's LDS), else in global scratch
    const void *rounds_fn = reinterpret_cast<const void *>(seqnms_rounds_kernel);
    const size_t ptr_bytes = (size_t)(Fmax * Rp + Fmax) * 2;
    size_t budget = kSqLdsBudget;
    if (c->max_lds < (size_t)kSqLdsBudget + 16384) budget = c->max_lds > 32768 ? c->max_lds - 16384 : 0;
    const bool lds = c->sq_lds && ptr_bytes <= budget;
    if (lds && !c->sq_attr_set) {
        HIPCHK(c, hipFuncSetAttribute(rounds_fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)budget));
        c->sq_attr_set = true;
    }
    HIPCHK(c, c->sq_link.reserve((size_t)(C * R * F * W) * 4));
    HIPCHK(c, c->sq_live.reserve((size_t)(C * F * W) * 4));
    HIPCHK(c, c->sq_done.reserve((size_t)(V * C) * 4));
    if (!lds) HIPCHK(c, c->sq_ptr.reserve((size_t)(C * F * (Rp + 1)) * 2));
    g.tracks = d_tracks; g.ntracks = d_ntracks; g.score = d_score; g.score_f64 = score_f64 ? 1 : 0;
    g.F = (int)Fmax; g.Ftot = (int)F; g.C = (int)C; g.R = R; g.W = (int)W; g.Rp = (int)Rp; g.S = max_seqs; g.rescore = rescore;
    g.rounds = (int)std::max<int64_t>(1, kSqFrameSteps / Fmax);
    g.ptr_lds = lds ? 1 : 0;
    g.link_t = link_thres; g.nms_t = nms_thres; g.min_score = min_score;
    g.otracks = d_tracks_out; g.oscore = d_score_out; g.oseq = d_seq_out; g.ontracks = d_ntracks_out; g.onseq = d_nseq;
    g.oseq_sum = d_seq_sum; g.oseq_len = d_seq_len; g.oseq_end = d_seq_end; g.oexh = d_exhausted;
    g.link = c->sq_link.as<uint32_t>(); g.live = c->sq_live.as<uint32_t>(); g.done = c->sq_done.as<int32_t>();
    g.gptr = lds ? nullptr : c->sq_ptr.as<int16_t>();
    c->sq_last_path = lds ? 1 : 2;
    {
        StageTimer tm(c, ST_TLINK);
        hipLaunchKernelGGL(seqnms_link_kernel, dim3((unsigned)(C * Fmax), (unsigned)V), dim3((unsigned)Rp), 0, c->stream, g);
    }
    {
        StageTimer tm(c, ST_TLOOP);
        const int launches = (max_seqs + 1 + g.rounds - 1) / g.rounds;      // (the + 1: the iteration that finds the rounds used up)
        for (int i = 0; i < launches; ++i)
            hipLaunchKernelGGL(seqnms_rounds_kernel, dim3((unsigned)C, (unsigned)V), dim3((unsigned)Rp), lds ? ptr_bytes : 0, c->stream, g);
    }
    HIPCHK(c, hipGetLastError());
    return VDET_OK;
}

int vdet_seq_nms(vdet_ctx *c, int64_t F, int64_t C, int R, const float *d_tracks, const int32_t *d_ntracks, const void *d_score,
                 int score_f64, double link_thres, double nms_thres, int rescore, int max_seqs, double min_score,
                 float *d_tracks_out, double *d_score_out, int32_t *d_seq_out, int32_t *d_ntracks_out, int32_t *d_nseq,
                 double *d_seq_sum, int32_t *d_seq_len, int32_t *d_seq_end, uint8_t *d_exhausted)
{
    const int64_t off[2] = {0, F};
    return vdet_seq_nms_batch(c, off, 1, C, R, d_tracks, d_ntracks, d_score, score_f64, link_thres, nms_thres, rescore, max_seqs,
                              min_score, d_tracks_out, d_score_out, d_seq_out, d_ntracks_out, d_nseq, d_seq_sum, d_seq_len,
                              d_seq_end, d_exhausted);
}

// ---------------------------------------------------------------------------------------------
// NMS over whole tubelets by spatio-temporal overlap (tubenms_kernels.hpp)
// ---------------------------------------------------------------------------------------------
int vdet_nms_tubelets_batch(vdet_ctx *c, const int64_t *h_frame_off, int64_t V, int64_t C, int T, const float *d_tracks,
                            const int32_t *d_ntracks, const float *d_tboxes, const void *d_score, int score_f64, int score_mode,
                            const float *d_anchors, const double *const *h_series, int n_series, double thresh, int norm,
                            int min_shared, float *d_tracks_out, int32_t *d_ntracks_out, float *d_tboxes_out, float *d_anchors_out,
                            double *d_series_out, int32_t *d_src, double *d_tscore, int32_t *d_by, double *d_overlaps)
{
    if (!c) return VDET_EINVAL;
    if (C < 1) return fail(c, VDET_EINVAL, "bad shape");
    if (T < 1 || T > kTubeMaxT) return fail(c, VDET_EINVAL, "T = %d tubelet slots per class; 1 .. %d", T, kTubeMaxT);
    if (n_series < 0 || n_series > kMergeMaxSeries) return fail(c, VDET_EINVAL, "0 to %d series", kMergeMaxSeries);
    if (thresh != thresh) return fail(c, VDET_EINVAL, "thresh must not be NaN");
    if (min_shared < 1) return fail(c, VDET_EINVAL, "min_shared must be at least 1");
    if (norm != VDET_TUBE_NORM_UNION && norm != VDET_TUBE_NORM_SHARED && norm != VDET_TUBE_NORM_MIN)
        return fail(c, VDET_EINVAL, "norm must be VDET_TUBE_NORM_UNION, VDET_TUBE_NORM_SHARED or VDET_TUBE_NORM_MIN");
    if (score_mode != VDET_TUBE_SCORE_SLOT && score_mode != VDET_TUBE_SCORE_MEAN && score_mode != VDET_TUBE_SCORE_MAX)
        return fail(c, VDET_EINVAL, "score_mode must be VDET_TUBE_SCORE_SLOT, VDET_TUBE_SCORE_MEAN or VDET_TUBE_SCORE_MAX");
    Videos vs;
    int rc = read_videos(c, h_frame_off, V, 65535, &vs);
    if (rc) return rc;
    if (!fits_below(0x7FFFFFF0ll, {C, T, vs.F}) || !fits_below(0x7FFFFFF0ll, {V, C, T}))
        return fail(c, VDET_EINVAL, "too many tubelet boxes (C*T*F must stay below 2^31 - 16)");
    if (!d_tracks || !d_ntracks || !d_score || !d_tracks_out || !d_ntracks_out || !d_src || !d_tscore || !d_by)
        return fail(c, VDET_EINVAL, "null buffer");
    if ((d_tboxes != nullptr) != (d_tboxes_out != nullptr)) return fail(c, VDET_EINVAL, "tboxes: the input and the output, or neither");
    if ((d_anchors != nullptr) != (d_anchors_out != nullptr)) return fail(c, VDET_EINVAL, "anchors: the input and the output, or neither");
    if (n_series && (!h_series || !d_series_out)) return fail(c, VDET_EINVAL, "null buffer");
    TubeArgs g{};
    for (int q = 0; q < n_series; ++q) {
        if (!h_series[q]) return fail(c, VDET_EINVAL, "null buffer");
        g.series[q] = h_series[q];
    }
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    if ((rc = video_table(c, c->anchor_tab, vs, &g.vids))) return rc;
    const int64_t W = (T + 31) / 32, slots = V * C * T;
    HIPCHK(c, c->tube_scratch.reserve((size_t)slots * (8 + 3 * 4 + (size_t)W * 4)));
    g.s.ts = c->tube_scratch.as<double>();
    g.s.n = reinterpret_cast<int32_t *>(g.s.ts + slots);
    g.s.first = g.s.n + slots;
    g.s.last = g.s.first + slots;
    g.s.bits = reinterpret_cast<uint32_t *>(g.s.last + slots);
    g.tracks = d_tracks; g.ntracks = d_ntracks; g.tboxes = d_tboxes; g.score = d_score; g.anchors = d_anchors;
    g.F = (int)vs.F; g.C = (int)C; g.T = T; g.W = (int)W; g.nser = n_series;
    g.score_f64 = score_f64 ? 1 : 0; g.score_mode = score_mode; g.norm = norm; g.min_shared = min_shared; g.thresh = thresh;
    g.otracks = d_tracks_out; g.ontracks = d_ntracks_out; g.oanchors = d_anchors_out; g.otboxes = d_tboxes_out;
    g.oseries = d_series_out; g.oN = C * T * vs.F; g.src = d_src; g.tscore = d_tscore; g.by = d_by; g.overlaps = d_overlaps;
    {
        StageTimer tm(c, ST_OTHER);
        const dim3 per_slot((unsigned)((C * T + kTubeWaves - 1) / kTubeWaves), (unsigned)V);
        const int64_t nt1 = (T + kTubeTile - 1) / kTubeTile, ntiles = nt1 * (nt1 + 1) / 2;      // (C * ntiles <= C * T)
        hipLaunchKernelGGL(tubenms_score_kernel, per_slot, dim3(kTubeLT), 0, c->stream, g);
        hipLaunchKernelGGL(tubenms_pair_kernel, dim3((unsigned)(C * ntiles), (unsigned)V), dim3(kTubeLT), 0, c->stream, g);
        hipLaunchKernelGGL(tubenms_select_kernel, dim3((unsigned)(V * C)), dim3(64), 0, c->stream, g);
        hipLaunchKernelGGL(tubenms_gather_kernel, per_slot, dim3(kTubeLT), 0, c->stream, g);
    }
    HIPCHK(c, hipGetLastError());
    return VDET_OK;
}

int vdet_nms_tubelets(vdet_ctx *c, int64_t F, int64_t C, int T, const float *d_tracks, const int32_t *d_ntracks,
                      const float *d_tboxes, const void *d_score, int score_f64, int score_mode, const float *d_anchors,
                      const double *const *h_series, int n_series, double thresh, int norm, int min_shared, float *d_tracks_out,
                      int32_t *d_ntracks_out, float *d_tboxes_out, float *d_anchors_out, double *d_series_out, int32_t *d_src,
                      double *d_tscore, int32_t *d_by, double *d_overlaps)
{
    const int64_t off[2] = {0, F};
    return vdet_nms_tubelets_batch(c, off, 1, C, T, d_tracks, d_ntracks, d_tboxes, d_score, score_f64, score_mode, d_anchors, h_series,
                                   n_series, thresh, norm, min_shared, d_tracks_out, d_ntracks_out, d_tboxes_out, d_anchors_out,
                                   d_series_out, d_src, d_tscore, d_by, d_overlaps);
}

}  // extern "C"
