"""Device-resident array forms of the hot path (torch tensors are only the memory / stream
plumbing; every computation is a gfx950 kernel behind the C-ABI of include/vdet_hip.h).

A c2-size video (300 frames x 10k boxes x 200 classes) cannot travel as protocol dicts (SURVEY
8a-a14: the JSON would be many GB); these functions are the array transport the dict-level API in
``vdetlib_amd.vdet`` is built on.
"""
import ctypes
import functools
import inspect
import itertools
import math

import numpy as np
import torch

from . import _lib


def _ctx_for(t, ctx=None):
    """The context to run on: the process-wide one of the tensor's device, or an explicit ``ctx``
    (one context per concurrently used HIP stream: a context owns its scratch buffers).  Either way
    the work is enqueued on torch's CURRENT stream."""
    if not t.is_cuda:
        raise ValueError("expected a CUDA/HIP tensor (vdetlib_amd has no CPU path)")
    if ctx is None:
        ctx = _lib.get_context(t.device.index if t.device.index is not None else torch.cuda.current_device())
    ctx.set_stream(torch.cuda.current_stream(t.device).cuda_stream)
    return ctx


def _finish(ctx, launch, sync, reset=None):
    """Enqueue ``launch()``; with ``sync`` wait for it -- and when an asynchronous context (``ctx.set_async``) reports
    that a graph build outgrew its scratch (``_lib.RetryError``: the scratch has been enlarged), restore the output
    buffers' initial state (``reset``) and enqueue once more."""
    launch()
    if sync:
        try:
            ctx.sync()
        except _lib.RetryError:
            ctx.invalidate()
            if reset is not None:
                reset()
            launch()
            ctx.sync()


def _keep_buffer(shape, device, pad):
    if pad:
        return torch.full(shape, -1, dtype=torch.int32, device=device)
    return torch.empty(shape, dtype=torch.int32, device=device)


def nms_volume(boxes, scores, thresh=0.3, score_thresh=None, cap=None, layout="FBC", sync=True, ctx=None, topk=0,
               pad=True):
    """Per-(frame, class) greedy NMS of a whole video (vdet/image_det.py:117-123 applied to every
    frame and class of vdet/video_det.py:89-99; == utils/nms.pyx vid_nms per class).

    boxes [F,B,4] f32, scores [F,B,C] (layout 'FBC', class innermost like zs[B,C]) or [F,C,B] ('FCB').
    score_thresh / topk: the candidate selection of fast_rcnn_det_vid (vdet/video_det.py:89-99:
    score > thresh, then the max_per_image best) on the device, before the NMS.
    Returns (keep_idx int32 [F,C,cap], keep_cnt int32 [F,C]); keep_idx[f,c,:cnt] are box indices in
    descending score order, the rest is -1 (pad=False: left uninitialised, saves one fill of the buffer).
    """
    boxes, scores, F, B, C = _volume(boxes, scores, layout=layout)
    lay = _lib.LAYOUT_FBC if layout == "FBC" else _lib.LAYOUT_FCB
    cap = B if cap is None else int(cap)
    ctx = _ctx_for(boxes, ctx)
    keep_idx = _keep_buffer((F, C, cap), boxes.device, pad)
    keep_cnt = torch.zeros((F, C), dtype=torch.int32, device=boxes.device)
    _finish(ctx, lambda: ctx.check(ctx.lib.vdet_nms_volume_topk(
        ctx.h, boxes.data_ptr(), scores.data_ptr(), lay, F, B, C, float(thresh), 0 if score_thresh is None else 1,
        0.0 if score_thresh is None else float(score_thresh), int(topk), keep_idx.data_ptr(), keep_cnt.data_ptr(), cap)), sync,
        reset=(lambda: keep_idx.fill_(-1)) if pad else None)
    return keep_idx, keep_cnt


def det_nms_volume(boxes, scores, score_thresh=0.05, topk=100, nms_thresh=0.3, first_class=1, sync=True, ctx=None,
                   want_dets=True):
    """The Fast R-CNN per-class flow of a whole video on the device: ``fast_rcnn_det_vid``'s per-class loop
    (vdet/video_det.py:89-99: ``scores[:, j] > thresh``, the ``max_per_image`` best, rows ``boxes[inds, 4j:4j+4] | score``)
    followed by ``apply_image_nms`` (vdet/image_det.py:117-123) for every frame and class -- every class suppresses its OWN
    regressed boxes (``nms_volume`` is the class-agnostic-box form).

    boxes [F,B,K,4] or [F,B,4K] f32 (the reference's per-frame ``[B, 4K]`` array), scores [F,B,K] f32; classes below
    ``first_class`` (the background column) are skipped.  ``score_thresh=None``: every box is a candidate.  Returns
      dets     [F,K,topk,5] f32 rows in the reference's row order (``all_boxes[j][i]`` = ``dets[i, j, :det_cnt[i, j]]``),
      sel_idx  [F,K,topk] int32 box index of every row,  det_cnt [F,K] int32,
      keep     [F,K,topk] int32 kept row positions, descending score (``apply_image_nms``'s list), keep_cnt [F,K] int32.
    Entries behind the counts are -1 (dets: NaN)."""
    if boxes.dtype != torch.float32 or scores.dtype != torch.float32:
        raise ValueError("Buffer dtype mismatch, expected 'float32_t'")
    scores = scores.contiguous()
    if scores.dim() != 3:
        raise ValueError("scores must be [F,B,K]")
    F, B, K = scores.shape
    boxes = boxes.contiguous()
    if tuple(boxes.shape) not in ((F, B, K, 4), (F, B, 4 * K)):
        raise ValueError("boxes must be [F,B,K,4] or [F,B,4K]")
    _same_gpu((boxes, scores), "boxes and scores")
    topk = int(topk)
    ctx = _ctx_for(boxes, ctx)
    dev = boxes.device
    dets = torch.full((F, K, topk, 5), float('nan'), dtype=torch.float32, device=dev) if want_dets else None
    sel = torch.full((F, K, topk), -1, dtype=torch.int32, device=dev)
    keep = torch.full((F, K, topk), -1, dtype=torch.int32, device=dev)
    det_cnt = torch.zeros((F, K), dtype=torch.int32, device=dev)
    keep_cnt = torch.zeros((F, K), dtype=torch.int32, device=dev)

    def reset():
        if dets is not None:
            dets.fill_(float('nan'))
        sel.fill_(-1); keep.fill_(-1)
    _finish(ctx, lambda: ctx.check(ctx.lib.vdet_det_nms_volume(
        ctx.h, boxes.data_ptr(), scores.data_ptr(), F, B, K, int(first_class), 0 if score_thresh is None else 1,
        0.0 if score_thresh is None else float(score_thresh), topk, float(nms_thresh),
        dets.data_ptr() if dets is not None else None, sel.data_ptr(), det_cnt.data_ptr(), keep.data_ptr(), keep_cnt.data_ptr())),
        sync, reset=reset)
    return dets, sel, det_cnt, keep, keep_cnt


def _im_size(im_size):
    try:
        H, W = (int(x) for x in im_size[:2])
    except (TypeError, ValueError):
        raise ValueError("im_size must be (H, W)")
    if H < 1 or W < 1:
        raise ValueError("im_size: H and W must be at least 1")
    return H, W


def _head_output(rois, deltas, lead, names):
    """K of a head's output: rois f32 / f64 ``lead + (4,)``, deltas f32 ``lead + (4K,)`` or ``lead + (K,4)`` (``lead``: the leading
    shape, or its rank when rois define it).  Layout only; ``names`` is the leading shape as the messages spell it."""
    if not torch.is_tensor(rois) or rois.dtype not in _F32_F64:
        raise ValueError("rois must be a float32 / float64 tensor")
    if not torch.is_tensor(deltas) or deltas.dtype != torch.float32:
        raise ValueError("deltas must be a float32 tensor")
    n = lead if isinstance(lead, int) else len(lead)
    if rois.dim() != n + 1 or rois.shape[-1] != 4 or (not isinstance(lead, int) and tuple(rois.shape[:n]) != tuple(lead)):
        raise ValueError("rois must be [%s,4]" % names)
    lead = tuple(rois.shape[:n])
    if deltas.dim() == n + 2 and tuple(deltas.shape[:n]) == lead and deltas.shape[-1] == 4:
        return int(deltas.shape[n])
    if deltas.dim() == n + 1 and tuple(deltas.shape[:n]) == lead and deltas.shape[-1] % 4 == 0:
        return int(deltas.shape[-1]) // 4
    raise ValueError("deltas must be [%s,4K] or [%s,K,4]" % (names, names))


def _aligned16(tensors, who):
    for t in tensors:
        if t is not None and t.numel() and t.data_ptr() % 16:
            raise ValueError("%s must be 16-byte aligned" % who)


def decode_boxes(rois, deltas, im_size, sync=True, ctx=None):
    """The Fast R-CNN box decode on the device (include/vdet_hip.h: vdet_decode_boxes): ``image_det.bbox_transform_inv``
    followed by ``clip_boxes`` for every box and class, one launch.

    rois [F,B,4] f32 / f64 (image coordinates, as they are), deltas [F,B,4K] or [F,B,K,4] f32 (the head's output), im_size
    (H, W).  Returns boxes [F,B,K,4] f32, the form ``det_nms_volume`` reads.  The arithmetic is float64, rounded once to float32,
    with an exponential that is a fixed sequence of IEEE operations: the bits are those of tests/decode_spec.py (against the
    host pair: at most one f32 ulp, on fewer than one element in 10^4).  A NaN stays a NaN; dw is not clamped.  rois and deltas
    must be 16-byte aligned (ValueError).  No CPU fallback."""
    K = _head_output(rois, deltas, 2, "F,B")
    H, W = _im_size(im_size)
    _same_gpu((rois, deltas), "rois and deltas")
    rois, deltas = rois.contiguous(), deltas.contiguous()
    _aligned16((rois, deltas), "rois and deltas")
    F, B = rois.shape[:2]
    boxes = torch.empty((F, B, K, 4), dtype=torch.float32, device=rois.device)
    ctx = _ctx_for(rois, ctx)
    ptr = lambda x: x.data_ptr() if x.numel() else None
    ctx.check(ctx.lib.vdet_decode_boxes(ctx.h, ptr(rois), int(rois.dtype == torch.float64), ptr(deltas), F * B, K, H, W, ptr(boxes)))
    if sync:
        ctx.sync()
    return boxes


def det_nms_volume_deltas(rois, scores, deltas, im_size, score_thresh=0.05, topk=100, nms_thresh=0.3, first_class=1, sync=True,
                          ctx=None, want_dets=True):
    """``det_nms_volume`` straight from the head's output (include/vdet_hip.h: vdet_det_nms_volume_deltas): the selection runs on
    the scores, and the wave of a (frame, class) decodes only its <= topk candidates, at the gather -- no [F,B,K,4] tensor exists.

    rois [F,B,4] f32 / f64, scores [F,B,K] f32, deltas [F,B,4K] or [F,B,K,4] f32, im_size (H, W); rois and deltas 16-byte
    aligned (ValueError).  Returns ``det_nms_volume``'s five outputs, bit for bit those of
    ``det_nms_volume(decode_boxes(rois, deltas, im_size), scores, ...)``, ZeroDivisionError and every error raised at the wait
    included.  The remaining arguments and the limits are ``det_nms_volume``'s.  Frames with fewer proposals: pad with NaN rois
    and NaN scores (a NaN never passes ``> score_thresh``).  No CPU fallback."""
    if not torch.is_tensor(scores) or scores.dtype != torch.float32:
        raise ValueError("Buffer dtype mismatch, expected 'float32_t'")
    if scores.dim() != 3:
        raise ValueError("scores must be [F,B,K]")
    F, B, K = scores.shape
    if _head_output(rois, deltas, (F, B), "F,B") != K:
        raise ValueError("deltas must be [F,B,4K] or [F,B,K,4] for scores [F,B,K]")
    H, W = _im_size(im_size)
    _same_gpu((rois, scores, deltas), "rois, scores and deltas")
    rois, scores, deltas = rois.contiguous(), scores.contiguous(), deltas.contiguous()
    _aligned16((rois, deltas), "rois and deltas")
    topk = int(topk)
    ctx = _ctx_for(rois, ctx)
    dev = rois.device
    dets = torch.full((F, K, topk, 5), float('nan'), dtype=torch.float32, device=dev) if want_dets else None
    sel = torch.full((F, K, topk), -1, dtype=torch.int32, device=dev)
    keep = torch.full((F, K, topk), -1, dtype=torch.int32, device=dev)
    det_cnt = torch.zeros((F, K), dtype=torch.int32, device=dev)
    keep_cnt = torch.zeros((F, K), dtype=torch.int32, device=dev)

    def reset():
        if dets is not None:
            dets.fill_(float('nan'))
        sel.fill_(-1); keep.fill_(-1)
    _finish(ctx, lambda: ctx.check(ctx.lib.vdet_det_nms_volume_deltas(
        ctx.h, rois.data_ptr(), int(rois.dtype == torch.float64), scores.data_ptr(), deltas.data_ptr(), F, B, K, H, W,
        int(first_class), 0 if score_thresh is None else 1, 0.0 if score_thresh is None else float(score_thresh), topk,
        float(nms_thresh), dets.data_ptr() if dets is not None else None, sel.data_ptr(), det_cnt.data_ptr(), keep.data_ptr(),
        keep_cnt.data_ptr())), sync, reset=reset)
    return dets, sel, det_cnt, keep, keep_cnt


def tubelet_dets(scores, deltas, tracks, slot, count, im_size, cols=None, shape=None, out=None, sync=True, ctx=None):
    """The tubelet side of the Fast R-CNN route after the head (include/vdet_hip.h: vdet_tubelet_dets; what ``fast_rcnn_cls``
    computes per tubelet box): for the compact row n of ``tubelet_rois`` with ``slot[n] = (c,t,f)``

        det[c,t,f] = f64(scores[n, cols[c]])        tboxes[c,t,f] = decode(tracks[c,t,f,:4], deltas[n, 4*cols[c] : +4])

    scores [N,K] f32 and deltas [N,4K] or [N,K,4] f32 are the head's output for the N pooled rows; tracks [C,T,F,>=4] f32 / f64;
    slot int32 [N,3] and count int32 [1] as ``tubelet_rois`` returns them (count None: all N; rows behind it are not read);
    ``cols`` int32 [C] maps a class to its column of the head as in ``svm_head`` (default c + 1: column 0 is the background).
    The decode is ``decode_boxes``' (tests/decode_spec.py).  ``shape`` = (C,T,F) defaults to tracks'.  ``out``: the dict of an
    earlier call, written in place at this call's slots only (frame ranges of one video); ``out=None`` allocates NaN.

    Returns a dict: ``det`` f64 [C,T,F] and ``tboxes`` f32 [C,T,F,4] -- what ``rescore_tubelets(floor=det)`` and
    ``nms_tracks(tboxes=)`` take.  A slot outside ``shape`` or a column outside K raises ValueError when the call -- with
    ``sync=False`` a later ``ctx.sync()`` -- waits; that row is skipped.  One launch.  No CPU fallback."""
    if not torch.is_tensor(scores) or scores.dtype != torch.float32 or scores.dim() != 2 or scores.shape[1] < 1:
        raise ValueError("scores must be float32 [N,K] with K >= 1")
    N, K = scores.shape
    if not torch.is_tensor(deltas) or deltas.dtype != torch.float32 or tuple(deltas.shape) not in ((N, 4 * K), (N, K, 4)):
        raise ValueError("deltas must be float32 [N,4K] or [N,K,4]")
    if not torch.is_tensor(tracks) or tracks.dtype not in _F32_F64 or tracks.dim() != 4 or tracks.shape[3] < 4:
        raise ValueError("tracks must be float32 / float64 [C,T,F,>=4]")
    if shape is not None and tuple(shape) != tuple(tracks.shape[:3]):
        raise ValueError("shape differs from tracks'")
    C, T, F, ld = (int(x) for x in tracks.shape)
    if C < 1 or T < 1 or F < 1 or C * T * F >= 2 ** 31 - 16:
        raise ValueError("shape must be C, T, F >= 1 with C*T*F below 2^31 - 16")
    if not torch.is_tensor(slot) or slot.dtype != torch.int32 or tuple(slot.shape) != (N, 3):
        raise ValueError("slot must be int32 [N,3]")
    if count is not None and (not torch.is_tensor(count) or count.dtype != torch.int32 or count.numel() != 1):
        raise ValueError("count must be int32 [1]")
    if cols is None:
        if C + 1 > K:
            raise ValueError("the default cols (c + 1) needs K >= C + 1 columns")
    elif not torch.is_tensor(cols) or cols.dtype != torch.int32 or tuple(cols.shape) != (C,):
        raise ValueError("cols must be int32 [C]")
    H, W = _im_size(im_size)
    if not all(x is None or x.is_contiguous() for x in (scores, deltas, tracks, slot, count, cols)):
        raise ValueError("scores, deltas, tracks, slot, count and cols must be contiguous")
    dev = scores.device
    if out is not None:
        if not isinstance(out, dict) or not torch.is_tensor(out.get('det')) or not torch.is_tensor(out.get('tboxes')):
            raise ValueError("out must be the dict of an earlier tubelet_dets call")
        det, tboxes = out['det'], out['tboxes']
        if det.dtype != torch.float64 or tuple(det.shape) != (C, T, F) or tboxes.dtype != torch.float32 or \
                tuple(tboxes.shape) != (C, T, F, 4) or not det.is_contiguous() or not tboxes.is_contiguous():
            raise ValueError("out's det must be float64 [C,T,F] and its tboxes float32 [C,T,F,4], contiguous")
    else:
        det = tboxes = None
    _same_gpu((scores, deltas, tracks, slot, count, cols, det, tboxes), "every tensor")
    if det is None:
        det = torch.full((C, T, F), float('nan'), dtype=torch.float64, device=dev)
        tboxes = torch.full((C, T, F, 4), float('nan'), dtype=torch.float32, device=dev)
    _aligned16((deltas, tboxes), "deltas and out's tboxes")
    ctx = _ctx_for(scores, ctx)
    ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None
    ctx.check(ctx.lib.vdet_tubelet_dets(ctx.h, ptr(scores), ptr(deltas), N, K, tracks.data_ptr(), int(tracks.dtype == torch.float64), ld,
                                        ptr(slot), ptr(count), C, T, F, ptr(cols), H, W, det.data_ptr(), tboxes.data_ptr()))
    if sync:
        ctx.sync()
    return dict(det=det, tboxes=tboxes)


def dets_as_tracks(dets, sel_idx, keep, keep_cnt, first_class=1, sync=True, ctx=None):
    """``det_nms_volume`` / ``det_nms_volume_deltas``' outputs in the rank layout ``nms_tracks`` returns (include/vdet_hip.h:
    vdet_dets_as_tracks): per-class regressed boxes as a source of everything that reads that layout.

    dets [F,K,topk,5] f32, sel_idx and keep [F,K,topk] int32, keep_cnt [F,K] int32.  With C = K - first_class and R = topk,
    returns the dict ``tracks`` [C,R,F,5] f32 (the kept rows of class first_class + c in keep order), ``score`` [C,R,F] f64,
    ``src`` [C,R,F] int32 (the row's box index; INT32_MIN behind the count), ``cnt`` [C,F] int32, ``ntracks`` [C] int32 (the
    maximum of cnt over the frames) -- NaN behind the counts.  It goes as it is into ``DetEvaluator.add_detections``,
    ``seq_nms`` and, as a tubelet dict, into ``nms_tracks`` / ``soft_nms_tracks`` / ``vote_nms_tracks`` (join it with real
    tubelets through ``merge_tracks('combine')`` first).  One launch.  No CPU fallback."""
    if not torch.is_tensor(dets) or dets.dtype != torch.float32 or dets.dim() != 4 or dets.shape[3] != 5:
        raise ValueError("dets must be float32 [F,K,topk,5] (det_nms_volume with want_dets=True)")
    F, K, R = (int(x) for x in dets.shape[:3])
    for t, name in ((sel_idx, "sel_idx"), (keep, "keep")):
        if not torch.is_tensor(t) or t.dtype != torch.int32 or tuple(t.shape) != (F, K, R):
            raise ValueError("%s must be int32 [F,K,topk]" % name)
    if not torch.is_tensor(keep_cnt) or keep_cnt.dtype != torch.int32 or tuple(keep_cnt.shape) != (F, K):
        raise ValueError("keep_cnt must be int32 [F,K]")
    first_class = int(first_class)
    if F < 1 or not 0 <= first_class < K:
        raise ValueError("F >= 1 frames and 0 <= first_class < K")
    if not 1 <= R <= 128:
        raise ValueError("topk = %d; the per-class NMS takes 1..128 boxes per (frame, class)" % R)
    if K * R * F >= 2 ** 31 - 16:
        raise ValueError("volume too large (K*topk*F must stay below 2^31 - 16)")
    _same_gpu((dets, sel_idx, keep, keep_cnt), "dets, sel_idx, keep and keep_cnt")
    dets, sel_idx, keep, keep_cnt = dets.contiguous(), sel_idx.contiguous(), keep.contiguous(), keep_cnt.contiguous()
    C, dev = K - first_class, dets.device
    out = dict(tracks=torch.empty((C, R, F, 5), dtype=torch.float32, device=dev),
               score=torch.empty((C, R, F), dtype=torch.float64, device=dev),
               src=torch.empty((C, R, F), dtype=torch.int32, device=dev),
               cnt=torch.empty((C, F), dtype=torch.int32, device=dev), ntracks=torch.empty((C,), dtype=torch.int32, device=dev))
    ctx = _ctx_for(dets, ctx)
    ctx.check(ctx.lib.vdet_dets_as_tracks(ctx.h, dets.data_ptr(), sel_idx.data_ptr(), keep.data_ptr(), keep_cnt.data_ptr(), F, K, R,
                                          first_class, out['tracks'].data_ptr(), out['score'].data_ptr(), out['src'].data_ptr(),
                                          out['cnt'].data_ptr(), out['ntracks'].data_ptr()))
    if sync:
        ctx.sync()
    return out


def generate_anchors(base_size=16, ratios=(0.5, 1, 2), scales=(8, 16, 32)):
    """The anchor table of a region proposal network on the host: float64 [A,4], ratio-major (A = len(ratios) * len(scales)),
    ``np.round`` on the ratio widths and heights -- tests/rpn_spec.py's function (the public py-faster-rcnn
    ``generate_anchors.py`` restated).  The defaults give the nine anchors (-84,-40,99,55) .. (-168,-344,183,359)."""
    ratios, scales = np.asarray(ratios, np.float64).reshape(-1), np.asarray(scales, np.float64).reshape(-1)
    size = np.float64(base_size)
    ctr = np.float64(0.5) * (size - 1)
    ws = np.round(np.sqrt(size * size / ratios))
    hs = np.round(ws * ratios)
    ws = (ws[:, None] * scales[None, :]).reshape(-1)
    hs = (hs[:, None] * scales[None, :]).reshape(-1)
    return np.stack([ctr - 0.5 * (ws - 1), ctr - 0.5 * (hs - 1), ctr + 0.5 * (ws - 1), ctr + 0.5 * (hs - 1)], axis=1)


RPN_MAX_ANCHORS, RPN_MAX_PRE = 64, 16384


def _rpn_common(scores, deltas, anchors, stride, pre, post, min_size, offset, dw_max):
    """The checks of rpn_proposals: (F, A, Hf, Wf, the scores' frame stride, anchors on the device, scalars)."""
    if not torch.is_tensor(scores) or scores.dtype != torch.float32 or scores.dim() != 4:
        raise ValueError("scores must be a float32 tensor [F,A,Hf,Wf]")
    if not torch.is_tensor(deltas) or deltas.dtype != torch.float32 or deltas.dim() != 4:
        raise ValueError("deltas must be a float32 tensor [F,4A,Hf,Wf]")
    F, A, Hf, Wf = scores.shape
    if tuple(deltas.shape) != (F, 4 * A, Hf, Wf):
        raise ValueError("deltas must be [F,4A,Hf,Wf] for scores [F,A,Hf,Wf]")
    if not scores.is_cuda:
        raise ValueError("expected a CUDA/HIP tensor (vdetlib_amd has no CPU path)")
    if not 1 <= A <= RPN_MAX_ANCHORS:
        raise ValueError("A = %d anchors per cell; 1 .. %d" % (A, RPN_MAX_ANCHORS))
    if Hf < 1 or Wf < 1 or Hf * Wf * A >= 2 ** 24:
        raise ValueError("the feature map must be Hf, Wf >= 1 with Hf*Wf*A below 2^24")
    if F * Hf * Wf * A >= 2 ** 31 - 16:
        raise ValueError("volume too large (F*Hf*Wf*A must stay below 2^31 - 16)")
    if torch.is_tensor(anchors):
        if anchors.dtype != torch.float64 or tuple(anchors.shape) != (A, 4):
            raise ValueError("anchors must be float64 [A,4]")
        if anchors.is_cuda and anchors.device != scores.device:
            raise ValueError("scores, deltas and anchors must be on the same GPU")
        anchors = anchors.to(scores.device).contiguous()
    else:
        anchors = np.asarray(anchors)
        if anchors.dtype != np.float64 or anchors.shape != (A, 4):
            raise ValueError("anchors must be float64 [A,4]")
        anchors = torch.from_numpy(np.array(anchors)).to(scores.device)
    if isinstance(stride, bool) or int(stride) != stride or int(stride) < 1 or int(stride) >= 2 ** 31:
        raise ValueError("stride must be an integer >= 1")
    if isinstance(pre, float) or isinstance(post, float) or not 1 <= int(post) <= int(pre) <= RPN_MAX_PRE:
        raise ValueError("1 <= post_nms_top_n <= pre_nms_top_n <= %d" % RPN_MAX_PRE)
    if F * int(pre) >= 2 ** 31 - 16:
        raise ValueError("volume too large (F*pre_nms_top_n must stay below 2^31 - 16)")
    min_size, offset = float(min_size), float(offset)
    if not math.isfinite(min_size) or not math.isfinite(offset):
        raise ValueError("min_size and offset must be finite")
    if dw_max is not None and math.isnan(float(dw_max)):
        raise ValueError("dw_max must not be NaN")
    # the foreground half cls[:, A:] of a contiguous [F,2A,Hf,Wf] tensor goes in as it is: only the frame stride is free
    st = scores.stride()
    if F * A * Hf * Wf and (st[1:] != (Hf * Wf, Wf, 1) or (F > 1 and st[0] < A * Hf * Wf)):
        scores = scores.contiguous()
    sstride = scores.stride(0) if F > 1 else A * Hf * Wf
    return scores, anchors, F, A, Hf, Wf, sstride, int(stride), int(pre), int(post), min_size, offset


def rpn_proposals(scores, deltas, anchors, im_size, stride=16, pre_nms_top_n=6000, post_nms_top_n=300, nms_thresh=0.7, min_size=16,
                  offset=1.0, dw_max=None, return_candidates=False, sync=True, ctx=None):
    """The proposal layer of a region proposal network on the device (include/vdet_hip.h: vdet_rpn_proposals): anchors, decode,
    clip, size filter, top-N, NMS, top-N for every frame of the call -- the boxes of the Faster R-CNN route.  The rule is
    tests/rpn_spec.py, bit for bit; it RESTATES the public py-faster-rcnn proposal layer, which was not at hand.

    scores [F,A,Hf,Wf] f32: the foreground scores, logits or probabilities (only the ranking is used); the slice ``cls[:, A:]``
    of a contiguous [F,2A,Hf,Wf] tensor is read in place.  deltas [F,4A,Hf,Wf] f32 (channel 4a+k: component k of anchor a),
    anchors float64 [A,4] (``generate_anchors``; numpy or tensor), im_size (H, W) of the network's input, ``stride`` the feature
    stride.  The candidate of flat index ``n = (h*Wf + w)*A + a`` is ``anchors[a] + (w,h,w,h)*stride`` decoded as
    ``decode_boxes`` does, with the width term ``(x2 - x1) + offset`` (1.0: the RPN's pixel convention; 1e-14 is
    ``decode_boxes``') and, with ``dw_max``, a dw / dh greater than it clamped to it.  It is valid when its score is not NaN and
    both sides of the clipped f32 box, plus 1, reach ``min_size``.  Valid candidates by descending score, equal scores by
    DESCENDING n; the first ``pre_nms_top_n`` (at most 16384) go through greedy NMS at ``nms_thresh`` (utils/nms.pyx's arithmetic)
    and the first ``post_nms_top_n`` survivors are the proposals.

    Returns a dict: ``rois`` [F,post,4] f32, ``scores`` [F,post] f32 (both NaN behind the count), ``index`` [F,post] int32 (n; -1
    behind the count), ``count`` [F] int32; with ``return_candidates`` also ``cand_index`` [F,pre] int32 (the candidates in
    order, -1 behind) and ``cand_cnt`` [F].  ``rois.view(-1, 4)`` with an image index feeds ``roi_pool`` (a NaN row: ok = 0 and a
    zero block), ``rois`` feeds ``det_nms_volume_deltas`` as its NaN-padded rois.  ValueError for a bad dtype, shape, device or
    limit, before any launch.  No CPU fallback."""
    H, W = _im_size(im_size)
    scores, anchors, F, A, Hf, Wf, sstride, stride, pre, post, min_size, offset = _rpn_common(
        scores, deltas, anchors, stride, pre_nms_top_n, post_nms_top_n, min_size, offset, dw_max)
    _same_gpu((scores, deltas), "scores and deltas")
    deltas = deltas.contiguous()
    dev = scores.device
    out = dict(rois=torch.empty((F, post, 4), dtype=torch.float32, device=dev),
               scores=torch.empty((F, post), dtype=torch.float32, device=dev),
               index=torch.empty((F, post), dtype=torch.int32, device=dev),
               count=torch.empty((F,), dtype=torch.int32, device=dev))
    if return_candidates:
        out['cand_index'] = torch.empty((F, pre), dtype=torch.int32, device=dev)
        out['cand_cnt'] = torch.empty((F,), dtype=torch.int32, device=dev)
    ctx = _ctx_for(scores, ctx)
    ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None
    _finish(ctx, lambda: ctx.check(ctx.lib.vdet_rpn_proposals(
        ctx.h, ptr(scores), sstride, ptr(deltas), ptr(anchors), F, A, Hf, Wf, H, W, stride, pre, post, float(nms_thresh), min_size,
        offset, 0 if dw_max is None else 1, 0.0 if dw_max is None else float(dw_max), ptr(out['rois']), ptr(out['scores']),
        ptr(out['index']), ptr(out['count']), ptr(out.get('cand_index')), ptr(out.get('cand_cnt')))), sync)
    return out


def nms_volume_ordered(boxes, order, ncand, thresh=0.3, cap=None, ctx=None, pad=True):
    """``nms_volume`` walking the CALLER's lists: order int16/uint16 [F,C,B] (box indices, e.g. ``argsort_volume``'s with
    ties rearranged as some machine's unstable ``scores.argsort()[::-1]`` left them, utils/nms.pyx:25), ncand int32 [F,C]
    (how many entries of each list are candidates).  Returns (keep_idx [F,C,cap], keep_cnt [F,C])."""
    F, B, _ = _volume_layout(boxes)
    if order.dtype not in (torch.int16, torch.uint16) or ncand.dtype != torch.int32 or order.dim() != 3 or \
            tuple(order.shape) != (F, order.shape[1], B) or tuple(ncand.shape) != (F, order.shape[1]):
        raise ValueError("order must be (u)int16 [F,C,B], ncand int32 [F,C], for boxes [F,B,4]")
    _same_gpu((boxes, order, ncand), "boxes, order and ncand")
    boxes, order, ncand = boxes.contiguous(), order.contiguous(), ncand.contiguous()
    C = order.shape[1]
    cap = B if cap is None else int(cap)
    ctx = _ctx_for(boxes, ctx)
    keep_idx = _keep_buffer((F, C, cap), boxes.device, pad)
    keep_cnt = torch.zeros((F, C), dtype=torch.int32, device=boxes.device)
    _finish(ctx, lambda: ctx.check(ctx.lib.vdet_nms_volume_ordered(
        ctx.h, boxes.data_ptr(), order.data_ptr(), ncand.data_ptr(), F, B, C, float(thresh), keep_idx.data_ptr(),
        keep_cnt.data_ptr(), cap)), True, reset=(lambda: keep_idx.fill_(-1)) if pad else None)
    return keep_idx, keep_cnt


def argsort_volume(scores, score_thresh=None, layout="FBC", ctx=None):
    """Descending argsort of every (frame, class) column of a score volume -- ``scores.argsort()[::-1]`` of
    utils/nms.pyx:25 / ``argsort(-cls_scores)`` of vdet/video_det.py:93 with the build's tie rule (equal scores by
    descending index, -0.0 == +0.0, NaN first).  Returns (order int16-as-uint16 [F,C,B] box indices, ncand int32 [F,C]);
    with score_thresh only boxes with score > score_thresh are candidates, the others form the tail."""
    if scores.dtype != torch.float32:
        raise ValueError("Buffer dtype mismatch, expected 'float32_t'")
    scores = scores.contiguous()
    if layout == "FBC":
        F, B, C = scores.shape
        lay = _lib.LAYOUT_FBC
    elif layout == "FCB":
        F, C, B = scores.shape
        lay = _lib.LAYOUT_FCB
    else:
        raise ValueError("layout must be 'FBC' or 'FCB'")
    ctx = _ctx_for(scores, ctx)
    order = torch.empty((F, C, B), dtype=torch.int16, device=scores.device)     # uint16 payload (B <= 32767: never negative)
    ncand = torch.zeros((F, C), dtype=torch.int32, device=scores.device)
    _finish(ctx, lambda: ctx.check(ctx.lib.vdet_argsort_volume(
        ctx.h, scores.data_ptr(), lay, F, B, C, 0 if score_thresh is None else 1,
        0.0 if score_thresh is None else float(score_thresh), order.data_ptr(), ncand.data_ptr())), True)
    return order, ncand


def temporal_maxpool(vol, window, pad=-1e5, ctx=None):
    """Centred sliding max along axis 0 (array form of score_proto_temporal_maxpool,
    vdet/tubelet_cls.py:386-414; pad value :402).  vol: f32 [F, ...]."""
    if window % 2 != 1:
        raise ValueError('Window size must be odd!')
    if vol.dtype != torch.float32:
        raise ValueError("Buffer dtype mismatch, expected 'float32_t'")
    vol = vol.contiguous()
    if window == 1:
        return vol.clone()          # (a copy like every other window size, never an alias of the input)
    out = torch.empty_like(vol)
    F = vol.shape[0]
    S = vol.numel() // F if F else 0
    ctx = _ctx_for(vol, ctx)
    ctx.check(ctx.lib.vdet_temporal_maxpool_f32(ctx.h, vol.data_ptr(), out.data_ptr(), F, S, int(window), float(pad)))
    return out


def temporal_conv(vol, taps, bias=0.0, pad=0.0, ctx=None):
    """Single-channel temporal convolution along axis 0 (build-defined stand-in for the external
    TCN of score_conv_cls, vdet/tubelet_cls.py:15-51): out[f] = bias + sum_k taps[k]*in[f+k-K/2]."""
    if vol.dtype != torch.float32:
        raise ValueError("Buffer dtype mismatch, expected 'float32_t'")
    vol = vol.contiguous()
    t = np.ascontiguousarray(taps, dtype=np.float32)
    out = torch.empty_like(vol)
    F = vol.shape[0]
    S = vol.numel() // F if F else 0
    ctx = _ctx_for(vol, ctx)
    ctx.check(ctx.lib.vdet_temporal_conv_f32(ctx.h, vol.data_ptr(), out.data_ptr(), F, S, t.ctypes.data,
                                             t.shape[0], float(bias), float(pad)))
    return out


def temporal_maxpool_conv(vol, window, taps, pad_max=-1e5, bias=0.0, pad_conv=0.0, ctx=None):
    """``temporal_maxpool(vol, window, pad_max)`` and ``temporal_conv(vol, taps, bias, pad_conv)`` (len(taps) ==
    window) in one pass over the volume (it is read once; the pass is HBM-bound).  Returns (pooled, conv)."""
    if window % 2 != 1:
        raise ValueError('Window size must be odd!')
    if vol.dtype != torch.float32:
        raise ValueError("Buffer dtype mismatch, expected 'float32_t'")
    t = np.ascontiguousarray(taps, dtype=np.float32)
    if t.shape[0] != window:
        raise ValueError('need one tap per window position')
    vol = vol.contiguous()
    out_m, out_c = torch.empty_like(vol), torch.empty_like(vol)
    F = vol.shape[0]
    S = vol.numel() // F if F else 0
    ctx = _ctx_for(vol, ctx)
    ctx.check(ctx.lib.vdet_temporal_maxpool_conv_f32(ctx.h, vol.data_ptr(), out_m.data_ptr(), out_c.data_ptr(), F, S,
                                                     int(window), float(pad_max), t.ctypes.data, float(bias), float(pad_conv)))
    return out_m, out_c


def volume_pass(scores, window=3, taps=None, pad_max=-1e5, bias=0.0, pad_conv=0.0, score_thresh=None, ctx=None, frame_off=None,
                out=None):
    """(``frame_off`` [V+1]: the volume is V videos concatenated along F -- a temporal window stops at its video's ends.)
    ONE read of a score volume [F,B,C]: ``temporal_maxpool(scores, window, pad_max)``, optionally
    ``temporal_conv(scores, taps, bias, pad_conv)`` (len(taps) == window), and -- left inside the context for
    the next ``nms_volume`` / ``track_volume`` / ``nms_track_volume`` call on the SAME scores tensor (cache
    enabled) -- the class-major sort keys of every (frame, class) problem (include/vdet_hip.h: vdet_volume_pass).
    Returns (pooled, conv or None).  ``out`` = (pooled buffer, conv buffer or None): caller-owned float32 tensors of at
    least ``scores.numel()`` elements to write into instead of fresh ones (a server keeps one pair per stream; the C-ABI
    takes caller buffers anyway); the returned tensors are views of them shaped like ``scores``."""
    if window % 2 != 1:
        raise ValueError('Window size must be odd!')
    if scores.dtype != torch.float32:
        raise ValueError("Buffer dtype mismatch, expected 'float32_t'")
    if scores.dim() != 3:
        raise ValueError("scores must be [F,B,C]")
    t = None
    if taps is not None:
        t = np.ascontiguousarray(taps, dtype=np.float32)
        if t.shape[0] != window:
            raise ValueError('need one tap per window position')
    scores = scores.contiguous()
    F, B, C = scores.shape
    ctx = _ctx_for(scores, ctx)
    if out is None:
        out_m = torch.empty_like(scores)
        out_c = torch.empty_like(scores) if t is not None else None
    else:
        def view(buf):
            if buf.dtype != torch.float32 or not buf.is_contiguous() or buf.numel() < scores.numel() or buf.device != scores.device:
                raise ValueError("out buffers must be contiguous float32 tensors of >= scores.numel() elements on the scores' device")
            return buf.view(-1)[:scores.numel()].view(scores.shape)
        if len(out) != 2 or out[0] is None or (t is not None and out[1] is None):
            raise ValueError("out = (pooled buffer, conv buffer): the conv buffer is needed when taps are given")
        out_m = view(out[0])
        out_c = view(out[1]) if t is not None else None
        # the kernel reads ``scores`` while it streams both outputs: overlapping buffers would give silently wrong results
        spans = [(b.data_ptr(), b.data_ptr() + scores.numel() * 4) for b in (scores, out_m, out_c) if b is not None]
        for i in range(len(spans)):
            for j in range(i + 1, len(spans)):
                if spans[i][0] < spans[j][1] and spans[j][0] < spans[i][1]:
                    raise ValueError("out buffers must not overlap each other or scores")
    tail = (int(window), float(pad_max), t.ctypes.data if t is not None else None, float(bias), float(pad_conv),
            out_m.data_ptr(), out_c.data_ptr() if out_c is not None else None, 0 if score_thresh is None else 1,
            0.0 if score_thresh is None else float(score_thresh))
    if frame_off is None:
        ctx.check(ctx.lib.vdet_volume_pass(ctx.h, scores.data_ptr(), F, B, C, *tail))
    else:
        off = _frame_offsets(frame_off, F)
        ctx.check(ctx.lib.vdet_volume_pass_batch(ctx.h, scores.data_ptr(), off.ctypes.data, len(off) - 1, B, C, *tail))
    return out_m, out_c


def _frame_offsets(frame_off, F=None):
    off = np.ascontiguousarray(frame_off, dtype=np.int64).reshape(-1)
    o = off.tolist()
    if len(o) < 2 or o[0] != 0 or (F is not None and o[-1] != F) or any(a >= e for a, e in zip(o, o[1:])):
        raise ValueError("frame_off must run 0 = o[0] < o[1] < ... < o[V]" + ("" if F is None else " = F"))
    return off


class _Batch(object):
    """The parsed form of a dict in ``video_batch``'s layout: what ``_batch_read`` returns."""
    __slots__ = ('off', 'o', 'V', 'Ft', 'C', 'T', 'tracks', 'ntracks', 'anchors', 'device')


_F32, _F64 = (torch.float32,), (torch.float64,)
_F32_F64 = _F32 + _F64


def _same_gpu(tensors, who, device=None):
    """ValueError unless every tensor lives on one GPU (``device``, or the first tensor's).  Called AFTER every layout check, so
    that a wrong layout fails as a layout whatever memory it is in."""
    device = tensors[0].device if device is None else device
    ok = device.type == 'cuda'
    for t in tensors:           # (None: an optional tensor that was not given)
        ok = ok and (t is None or t.device == device)
    if not ok:
        raise ValueError("%s must live on the same GPU (vdetlib_amd has no CPU path)" % who)


# ---- the checked readers of the entry points' inputs.  Attribute checks only (no device query, no copy to the host): the batch
# routes pay them per call.  All but ``_volume`` check the LAYOUT only; the entry point follows with ONE ``_same_gpu`` (or ends
# with ``_volume``, which takes the tensors read so far as ``also``), so that nothing reaches a kernel from the wrong memory.
def _volume_layout(boxes, scores=None, layout="FBC", F=None, C=None, nonempty=False):
    """(F, B, C) of a video's detections: boxes f32 [F,B,4] and -- unless None -- scores f32 [F,B,C] ('FCB': [F,C,B]), checked
    against each other and against a given ``F`` / ``C``; ``nonempty``: at least one frame, box and class."""
    bs = boxes.shape
    if boxes.dtype != torch.float32 or len(bs) != 3 or bs[2] != 4 or (F is not None and bs[0] != F):
        raise ValueError("boxes must be float32 [F,B,4]" + ("" if F is None else " with F = %d" % F))
    F, B = bs[0], bs[1]
    if scores is not None:
        if layout not in ("FBC", "FCB"):
            raise ValueError("layout must be 'FBC' or 'FCB'")
        ss = scores.shape
        Cs = ss[2 if layout == "FBC" else 1] if len(ss) == 3 else None
        if scores.dtype != torch.float32 or ss != ((F, B, Cs) if layout == "FBC" else (F, Cs, B)) or (C is not None and Cs != C):
            raise ValueError("scores must be float32 [%s] for boxes [%d,%d,4]%s" % (
                ','.join(layout), F, B, "" if C is None else " with C = %d" % C))
        C = Cs
    if nonempty and (F < 1 or B < 1 or (scores is not None and C < 1)):
        raise ValueError("boxes%s must hold at least one frame, one box per frame%s" % (
            ("", "") if scores is None else (" and scores", " and one class")))
    return F, B, C


def _volume(boxes, scores, also=(), who="boxes and scores", layout="FBC", F=None, C=None, nonempty=False):
    """The reader of a volume that goes to a kernel: ``_volume_layout``, then boxes, scores and the tensors of the tuple ``also``
    (whose layout the caller has checked) on one GPU.  Returns (boxes, scores, F, B, C), the tensors contiguous."""
    F, B, C = _volume_layout(boxes, scores, layout, F, C, nonempty)
    _same_gpu((boxes, scores) + also, who)
    return boxes.contiguous(), scores.contiguous(), F, B, C


def _tubelets_layout(tracks, ntracks, anchors=None):
    """(C, T, F) of one video's tubelets: tracks f32 [C,T,F,5], ntracks int32 [C] and -- unless None -- anchors f32 [C,T,3]."""
    ts = tracks.shape
    if tracks.dtype != torch.float32 or len(ts) != 4 or ts[3] != 5:
        raise ValueError("tracks must be float32 [C,T,F,5]")
    if ntracks.dtype != torch.int32 or ntracks.shape != ts[:1]:
        raise ValueError("ntracks must be int32 [C]")
    if anchors is not None and (anchors.dtype != torch.float32 or anchors.shape != (ts[0], ts[1], 3)):
        raise ValueError("anchors must be float32 [C,T,3]")
    return ts[0], ts[1], ts[2]


def _anchor_slots(anchor_frames, anchor_boxes, anchor_scores=None, V=None):
    """Caller-supplied anchors: anchor_frames int32 [C,T], anchor_boxes f32 [C,T,4], anchor_scores f32 [C,T] or None -- with
    ``V`` all under a leading [V,...].  Returns them contiguous, and C, T."""
    lead, nd = ("C,T", 2) if V is None else ("V,C,T", 3)
    if anchor_frames.dtype != torch.int32 or anchor_frames.dim() != nd or (V is not None and anchor_frames.shape[0] != V) or \
            anchor_frames.shape[-2] < 1:
        raise ValueError("anchor_frames must be int32 [%s] with C >= 1" % lead)
    shape = tuple(anchor_frames.shape)
    if anchor_boxes.dtype != torch.float32 or anchor_boxes.shape != shape + (4,):
        raise ValueError("anchor_boxes must be float32 [%s,4]" % lead)
    if anchor_scores is not None and (anchor_scores.dtype != torch.float32 or anchor_scores.shape != shape):
        raise ValueError("anchor_scores must be float32 [%s] or None" % lead)
    return (anchor_frames.contiguous(), anchor_boxes.contiguous(), None if anchor_scores is None else anchor_scores.contiguous(),
            shape[-2], shape[-1])


def _images(images):
    """(F, H, W) of the frames images uint8 [F,H,W,3]: contiguous, at least one frame, 1 .. 32767 rows and columns."""
    if not torch.is_tensor(images) or images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3 or \
            not images.is_contiguous():
        raise ValueError("images must be uint8 [F,H,W,3], contiguous")
    F, H, W = images.shape[:3]
    if F < 1 or not 1 <= H <= 32767 or not 1 <= W <= 32767:
        raise ValueError("images must hold at least one frame of 1 .. 32767 rows and columns, not [%d,%d,%d,3]" % (F, H, W))
    return F, H, W


def _pixel_settings(grid, radius, min_conf, max_frames, step):
    """the five checked settings of the pixel tracker, in the order of the C-ABI's arguments"""
    grid, radius, max_frames, step, min_conf = int(grid), int(radius), int(max_frames), int(step), float(min_conf)
    if grid % 4 or not 4 <= grid <= 64:
        raise ValueError("grid = %d; a multiple of 4 in 4 .. 64" % grid)
    if not 1 <= radius <= 16:
        raise ValueError("radius = %d; 1 .. 16" % radius)
    if step < 1 or max_frames < 0:
        raise ValueError("step must be >= 1 and max_frames >= 0")
    if not math.isfinite(min_conf):
        raise ValueError("min_conf must be finite")
    return grid, radius, min_conf, max_frames, step


def _pixel_sampling(sampling, integral, images, F, H, W):
    """The checked ``sampling`` / ``integral`` pair of a pixel-tracker call: True for 'box'.  Layout checks only; the entry
    point's ``_same_gpu`` takes the integral with the other tensors."""
    if sampling not in ('point', 'box'):
        raise ValueError("sampling = %r; 'point' or 'box'" % (sampling,))
    if sampling == 'point':
        if integral is not None:
            raise ValueError("an integral is read by sampling='box' only")
        return False
    if H * W > 1 << 24:
        raise ValueError("sampling='box': frames of at most 2^24 pixels, not %d x %d" % (H, W))
    if integral is not None and (not torch.is_tensor(integral) or integral.dtype != torch.uint32 or
                                 tuple(integral.shape) != (F, H + 1, W + 1) or not integral.is_contiguous()):
        raise ValueError("integral must be uint32 [F,H+1,W+1] = [%d,%d,%d], contiguous (ops.luma_integral of the images)" % (F, H + 1, W + 1))
    return True


def luma_integral(images, sync=True, ctx=None):
    """The integral image (summed-area table) of every frame's luma, the input of the pixel tracker's ``sampling='box'``
    (include/vdet_hip.h: vdet_luma_integral; the rule is tests/pixtrack_spec.py): build it once per video and pass it as
    ``integral=`` to as many tracker calls as read that video.

    images uint8 [F,H,W,3], contiguous, H*W <= 2^24 -> uint32 [F,H+1,W+1] on the images' GPU:
    out[f, y, x] = sum of L[f, r, c] over r < y, c < x with L = (29*c0 + 150*c1 + 77*c2 + 128) >> 8; row 0 and column 0 are
    zero.  Exact.  Two launches, no host wait; 4/3 of the images' bytes.  ValueError for images of another layout or of more
    than 2^24 pixels a frame (before any launch)."""
    F, H, W = _images(images)
    _pixel_sampling('box', None, images, F, H, W)
    ctx = _ctx_for(images, ctx)
    out = torch.empty((F, H + 1, W + 1), dtype=torch.uint32, device=images.device)
    ctx.check(ctx.lib.vdet_luma_integral(ctx.h, images.data_ptr(), F, H, W, out.data_ptr()))
    if sync:
        ctx.sync()
    return out


def _track_outputs(C, T, F, device, early_stop, V=None):
    """The tracks / anchors / ntracks outputs of a tracker: [C,T,F,5] f32, [C,T,3] f32, [C] int32 -- with ``V`` in
    ``video_batch``'s layout: flat tracks, [V,C,T,3], [V,C].  ``early_stop``: the call may end before it has written every
    slot, so they start as NaN, zero, zero; a call that writes every element takes them uninitialised."""
    lead = (C,) if V is None else (V, C)
    shape = (C, T, F, 5) if V is None else (C * T * F * 5,)
    if not early_stop:
        return (torch.empty(shape, dtype=torch.float32, device=device), torch.empty(lead + (T, 3), dtype=torch.float32, device=device),
                torch.empty(lead, dtype=torch.int32, device=device))
    return (torch.full(shape, float('nan'), dtype=torch.float32, device=device),
            torch.zeros(lead + (T, 3), dtype=torch.float32, device=device), torch.zeros(lead, dtype=torch.int32, device=device))


def _batch_views(flat, off, C, T, per):
    """The per-video views of one flat buffer in ``video_batch``'s layout (``_batch_read``): [C,T,F_v] for ``per`` == 1, else
    [C,T,F_v,per]; video v starts at element C*T*per*off[v].  Each view is made by ONE as_strided call with the strides of a
    contiguous tensor of its shape (torch counts an empty axis as 1: max(T, 1)) -- the same tensor as
    ``flat[n*off[v]:n*off[v+1]].view(C, T, F_v, per)`` at half the host time, which the batches of many videos need."""
    o, base = off.tolist(), flat.storage_offset()
    shape, strides = ((per,), (per, 1)) if per > 1 else ((), (1,))
    return [flat.as_strided((C, T, e - a) + shape, (max(T, 1) * (e - a) * per, (e - a) * per) + strides, base + C * T * per * a)
            for a, e in zip(o, o[1:])]


def _batch_field(b, views, per, dtypes, name, who, T=None, gather=False, axis=False, shapes=True):
    """One field of a dict in ``video_batch``'s layout, checked against the batch ``b`` (``_batch_read``) and returned as its
    flat buffer, with no copy: ``views`` must be b.V tensors of ONE of ``dtypes``, view v [C,T,F_v] for ``per`` == 1 (with
    ``axis``: [C,T,F_v,1], the rows of a wide blob), else [C,T,F_v,per], with ``T`` slots (default b.T); every view contiguous
    and exactly at element C*T*per*off[v] behind the first, all in one allocation (so on one device).  ``gather``: views of the
    right shapes and dtype that are not such slices are copied into one buffer instead of refused.  One pass over the views;
    the text of an error is made only when there is one."""
    if T is None:
        T = b.T
    C, o = b.C, b.o
    four = axis or per > 1
    ok = isinstance(views, (list, tuple)) and len(views) == b.V and isinstance(views[0], torch.Tensor) and views[0].dtype in dtypes
    if ok:
        first = views[0]
        dtype, p0, step, near = first.dtype, first.data_ptr(), C * T * per * first.element_size(), True
        for x, a, e in zip(views, o, o[1:]):
            if not isinstance(x, torch.Tensor) or x.dtype != dtype or \
                    (shapes and x.shape != ((C, T, e - a, per) if four else (C, T, e - a))):
                ok = False
                break
            near = near and x.is_contiguous() and x.data_ptr() == p0 + step * a
    if not ok:
        raise ValueError(_batch_field_error(b, views, per, dtypes, name, who, T, four, shapes))
    if near:
        try:
            return torch.as_strided(first, (C * T * per * b.Ft,), (1,))
        except RuntimeError:       # neighbours by address, but past the end of the first view's storage
            pass
    if not gather:
        raise ValueError("%s: the views of %s are not contiguous, consecutive slices of one allocation" % (who, name))
    return torch.cat([x.reshape(-1) for x in views])


def _batch_field_error(b, views, per, dtypes, name, who, T, four, shapes):
    what = "%s: %s must be %s [C,T,F_v%s] views in video_batch's layout, one per video" % (
        who, name, ' / '.join(str(d).replace('torch.', '') for d in dtypes), ',%d' % per if four else '')
    if isinstance(views, (list, tuple)) and len(views) == b.V:
        for v, x in enumerate(views):
            want = (b.C, T, b.o[v + 1] - b.o[v]) + ((per,) if four else ())
            if not isinstance(x, torch.Tensor) or x.dtype not in dtypes or x.dtype != views[0].dtype or (shapes and x.shape != want):
                return "%s; %s[%d] must be %s of the one dtype, not %s" % (
                    what, name, v, list(want), "%s %s" % (x.dtype, list(x.shape)) if isinstance(x, torch.Tensor) else type(x).__name__)
    return what


def _batch_flat(views, per=None):
    """The flat buffer behind per-video views in ``video_batch``'s layout when there is no batch to check their shapes
    against (``per`` is not used): ``_batch_field``'s checks with every view beginning where its predecessor ends."""
    if not isinstance(views, (list, tuple)) or not views or not all(isinstance(x, torch.Tensor) for x in views):
        raise ValueError("not a video_batch result: the per-video views must be a list of tensors")
    b = _Batch()
    b.o = [0] + list(itertools.accumulate(x.numel() for x in views))
    b.V, b.Ft, b.C, b.T = len(views), b.o[-1], 1, 1
    return _batch_field(b, views, 1, (views[0].dtype,), 'the per-video list', 'not a video_batch result', shapes=False)


def _batch_read(bo, who='batch_out', need=()):
    """The one reader of "a dict in ``video_batch``'s layout", the form in which ``video_batch``, ``track_from_anchors_batch``,
    ``anchor_propagate_tracks_batch``, ``tcn_tracks_batch``, ``interpolate_tracks_batch``, ``merge_tracks_batch``,
    ``nms_tracks_batch``, ``rescore_tubelets_batch``, ``tubelets_overlap_batch`` and ``DetEvaluator.add_batch`` /
    ``add_detections`` hand V videos' tubelets to each other.  The layout:
      frame_off   [V+1] offsets, 0 = o[0] < o[1] < ... < o[V] = F_total: video v owns the frames o[v] .. o[v+1] (F_v of them);
      tracks      a list of V views [C,T,F_v,5] f32;  det / pooled / score / ... [C,T,F_v] and tboxes [C,T,F_v,4] likewise.
                  The views of one field are CONSECUTIVE slices of ONE flat allocation: video v starts at element
                  C*T*per*o[v] (per = 5, 1, 4: the width of a box's entry), which is how the kernels index the field from one
                  pointer.  ``_batch_views`` builds such lists, ``_batch_field`` checks one and returns the flat buffer;
      ntracks     [V,C] int32;  anchors [V,C,T,3] f32.
    It is a plain dict: callers may build one by hand.  Everything is CHECKED BEFORE ANY LAUNCH, on the host and in this order:
    the dict has ``tracks``, ``ntracks``, ``frame_off`` and the keys of ``need`` (an empty list is a missing field); frame_off;
    V <= 65535; tracks (shapes, dtype, consecutive views); ntracks; anchors when needed.  ValueError otherwise -- a view that is
    not where the layout puts it would be read from the wrong memory, or past the end of it.  Returns a ``_Batch``: off
    (contiguous int64), o (off as a list of ints), V, Ft, C, T, the flat tracks, ntracks (contiguous), anchors (contiguous, None
    unless needed) and the device."""
    keys = ('tracks', 'ntracks', 'frame_off') + need
    missing = not isinstance(bo, dict)
    for k in () if missing else keys:
        x = bo.get(k)
        missing = missing or x is None or (isinstance(x, (list, tuple)) and not x)
    if missing:
        raise ValueError("%s is not a video_batch result: it must be a dict in video_batch's layout with %s" % (who, ', '.join(keys)))
    b = _Batch()
    b.off = _frame_offsets(bo['frame_off'])
    b.o = b.off.tolist()
    V, tv = len(b.o) - 1, bo['tracks']
    if V > 65535:
        raise ValueError("at most 65535 videos in one call")
    bad = "%s is not a video_batch result" % who
    if not isinstance(tv, (list, tuple)) or not isinstance(tv[0], torch.Tensor) or tv[0].dim() != 4:
        raise ValueError("%s: tracks must be a list of float32 [C,T,F_v,5] views" % bad)
    shape = tv[0].shape
    b.V, b.Ft, b.C, b.T, b.device = V, b.o[-1], shape[0], shape[1], tv[0].device
    b.tracks = _batch_field(b, tv, 5, _F32, 'tracks', bad)
    ntracks = bo['ntracks']
    if not isinstance(ntracks, torch.Tensor) or ntracks.dtype != torch.int32 or ntracks.shape != (V, b.C):
        raise ValueError("%s: ntracks must be int32 [V,C]" % bad)
    b.ntracks, b.anchors = ntracks.contiguous(), None
    if 'anchors' in need:
        anchors = bo['anchors']
        if not isinstance(anchors, torch.Tensor) or anchors.dtype != torch.float32 or anchors.shape != (V, b.C, b.T, 3):
            raise ValueError("%s: anchors float32 [V,C,T,3] are needed" % bad)
        b.anchors = anchors.contiguous()
    return b


def video_batch(boxes, scores, frame_off, nms_thres=0.3, thres=0.0, max_tracks=10, link_thres=0.5, max_frames=0, cap=None,
                nms=True, rescore=True, overlap_thres=0.7, window=3, sync=True, ctx=None, pad=True):
    """V small videos in ONE call (include/vdet_hip.h: vdet_video_batch): boxes [F,B,4] / scores [F,B,C] hold the frames
    of all videos one after the other, ``frame_off`` [V+1] their frame ranges.  Per video the results are what
    ``nms_track_volume`` + ``rescore_tracks`` return for it alone.  Returns a dict in the batch layout (``_batch_read``):
    tracks, det / pooled f64 and tboxes (rescore; else empty lists), anchors, ntracks, frame_off -- plus keep_idx [F,C,cap] /
    keep_cnt [F,C] (nms)."""
    F, B, C = _volume_layout(boxes, scores)
    off = _frame_offsets(frame_off, F)
    _same_gpu((boxes, scores), "boxes and scores")
    boxes, scores = boxes.contiguous(), scores.contiguous()
    V, T = len(off) - 1, int(max_tracks)
    ctx = _ctx_for(boxes, ctx)
    dev = boxes.device
    cap = B if cap is None else int(cap)
    keep_idx = _keep_buffer((F, C, cap), dev, pad) if nms else None
    keep_cnt = torch.zeros((F, C), dtype=torch.int32, device=dev) if nms else None
    tracks, anchors, ntracks = _track_outputs(C, max(T, 1), F, dev, True, V=V)
    det = torch.empty((C * max(T, 1) * F,), dtype=torch.float64, device=dev) if rescore else None
    pooled = torch.empty_like(det) if rescore else None
    tboxes = torch.empty((C * max(T, 1) * F * 4,), dtype=torch.float32, device=dev) if rescore else None

    def launch():
        ctx.check(ctx.lib.vdet_video_batch(
            ctx.h, boxes.data_ptr(), scores.data_ptr(), off.ctypes.data, V, B, C, float(nms_thres), float(thres), T, float(link_thres),
            int(max_frames), tracks.data_ptr(), anchors.data_ptr(), ntracks.data_ptr(), cap,
            keep_idx.data_ptr() if nms else None, keep_cnt.data_ptr() if nms else None, float(overlap_thres), int(window),
            det.data_ptr() if rescore else None, pooled.data_ptr() if rescore else None, tboxes.data_ptr() if rescore else None))

    def reset():
        tracks.fill_(float('nan'))
        if nms and pad:
            keep_idx.fill_(-1)

    _finish(ctx, launch, sync, reset=reset)
    out = dict(keep_idx=keep_idx, keep_cnt=keep_cnt, anchors=anchors[:, :, :T], ntracks=ntracks, frame_off=off)
    views = lambda flat, per: _batch_views(flat, off, C, T, per) if flat is not None else []
    out.update(tracks=views(tracks, 5), det=views(det, 1), pooled=views(pooled, 1), tboxes=views(tboxes, 4))
    return out


def iou(boxes1, boxes2):
    """utils/common.py:451-468 -- float64 IoU matrix [n1,n2] (+1 convention), numpy in / numpy out."""
    b1 = np.ascontiguousarray(np.asarray(boxes1).astype('float'))
    b2 = np.ascontiguousarray(np.asarray(boxes2).astype('float'))
    if b1.ndim != 2 or b2.ndim != 2 or b1.shape[1] < 4 or b2.shape[1] < 4:
        raise IndexError("boxes must be [n,4]")
    b1 = np.ascontiguousarray(b1[:, :4])
    b2 = np.ascontiguousarray(b2[:, :4])
    out = np.empty((b1.shape[0], b2.shape[0]), dtype=np.float64)
    if out.size:
        ctx = _lib.get_context()
        ctx.reset_stream()
        ctx.check(ctx.lib.vdet_iou_f64(ctx.h, b1.ctypes.data, b1.shape[0], b2.ctypes.data, b2.shape[0],
                                       out.ctypes.data))
    return out


def track_volume(boxes, scores, nms_thres=0.3, thres=0.0, max_tracks=10, link_thres=0.5, max_frames=0, sync=True,
                 ctx=None):
    """Greedy tubelet generation for EVERY class of a video on the GPU: the array form of
    greedily_track_from_raw_dets (vdet/track.py:189-252) with the built-in IoU-linking tracker as
    ``track_method`` (the reference's trackers are external MATLAB code).

    boxes [F,B,4] f32, scores [F,B,C] f32.  Returns
      tracks  [C, max_tracks, F, 5] f32 rows (x1,y1,x2,y2,score), NaN where a track has no box,
      anchors [C, max_tracks, 3] f32 (1-based frame, box index, score),  ntracks [C] int32."""
    boxes, scores, F, B, C = _volume(boxes, scores)
    ctx = _ctx_for(boxes, ctx)
    tracks, anchors, ntracks = _track_outputs(C, max_tracks, F, boxes.device, True)
    _finish(ctx, lambda: ctx.check(ctx.lib.vdet_track_volume(
        ctx.h, boxes.data_ptr(), scores.data_ptr(), F, B, C, float(nms_thres), float(thres), int(max_tracks),
        float(link_thres), int(max_frames), tracks.data_ptr(), anchors.data_ptr(), ntracks.data_ptr())), sync,
        reset=lambda: (tracks.fill_(float('nan')), anchors.zero_()))
    return tracks, anchors, ntracks


def nms_track_volume(boxes, scores, nms_thres=0.3, thres=0.0, max_tracks=10, link_thres=0.5, max_frames=0, cap=None,
                     sync=True, ctx=None, pad=True, keep_out=None):
    """``nms_volume`` (layout 'FBC', no score threshold) and ``track_volume`` of the same video in one
    call: both are greedy walks over the same sorted lists and suppression graph, and on regular
    videos one fused walk serves both (include/vdet_hip.h: vdet_nms_track_volume).  Results are
    bit-identical to the two separate calls.  ``keep_out``: a caller-owned contiguous int32 tensor of >= F*C*cap elements
    to hold keep_idx (the returned keep_idx is a view of it).
    Returns (keep_idx, keep_cnt, tracks, anchors, ntracks)."""
    boxes, scores, F, B, C = _volume(boxes, scores)
    cap = B if cap is None else int(cap)
    ctx = _ctx_for(boxes, ctx)
    if keep_out is None:
        keep_idx = _keep_buffer((F, C, cap), boxes.device, pad)
    else:
        if keep_out.dtype != torch.int32 or not keep_out.is_contiguous() or keep_out.numel() < F * C * cap or keep_out.device != boxes.device:
            raise ValueError("keep_out must be a contiguous int32 tensor of >= F*C*cap elements on the boxes' device")
        keep_idx = keep_out.view(-1)[:F * C * cap].view(F, C, cap)
        if pad:
            keep_idx.fill_(-1)
    keep_cnt = torch.zeros((F, C), dtype=torch.int32, device=boxes.device)
    tracks, anchors, ntracks = _track_outputs(C, max_tracks, F, boxes.device, True)
    _finish(ctx, lambda: ctx.check(ctx.lib.vdet_nms_track_volume(
        ctx.h, boxes.data_ptr(), scores.data_ptr(), F, B, C, float(nms_thres), float(thres), int(max_tracks),
        float(link_thres), int(max_frames), tracks.data_ptr(), anchors.data_ptr(), ntracks.data_ptr(), cap,
        keep_idx.data_ptr(), keep_cnt.data_ptr())), sync,
        reset=lambda: (keep_idx.fill_(-1) if pad else None, tracks.fill_(float('nan')), anchors.zero_()))
    return keep_idx, keep_cnt, tracks, anchors, ntracks


def tracks_to_proto(video_name, tracks, anchors, ntracks, method='iou_link_tracker'):
    """One class's device tracks -> a .track protocol dict (utils/protocol.py:389-414 fields)."""
    from .utils.protocol import bbox_hash
    tr = tracks.cpu().numpy() if hasattr(tracks, 'cpu') else np.asarray(tracks)
    an = anchors.cpu().numpy() if hasattr(anchors, 'cpu') else np.asarray(anchors)
    out = []
    for t in range(int(ntracks)):
        anchor_frame = int(an[t, 0])
        tracklet = []
        for f in range(tr.shape[1]):
            row = tr[t, f]
            if np.isnan(row[0]):
                continue
            bbox = [int(v) for v in row[:4]]
            tracklet.append({'frame': f + 1, 'bbox': bbox, 'hash': bbox_hash(video_name, f + 1, row),
                             'score': float(row[4]), 'anchor': int(f + 1 - anchor_frame)})
        out.append(tracklet)
    return {'video': video_name, 'method': method, 'tracks': out}


def rescore_tracks(tracks, ntracks, boxes, scores, overlap_thres=0.7, window=3, sync=True, ctx=None):
    """Re-score device tracks: spatial max-pooling of the detection scores onto the tubelet boxes
    (raw_dets_spatial_max_pooling, vdet/tubelet_cls.py:493-535 -- also replaces each box by the
    best-scoring overlapping detection), gap completion (:284-303) and temporal max-pooling
    (:386-414).  Returns (det_score f64 [C,T,F], pooled f64 [C,T,F], boxes f32 [C,T,F,4])."""
    if window % 2 != 1:
        raise ValueError('Window size must be odd!')
    C, T, F = _tubelets_layout(tracks, ntracks)
    boxes, scores, F, B, C = _volume(boxes, scores, (tracks, ntracks), "tracks, ntracks, boxes and scores", F=F, C=C)
    ntracks = ntracks.contiguous()
    ctx = _ctx_for(boxes, ctx)
    det = torch.empty((C, T, F), dtype=torch.float64, device=boxes.device)
    pooled = torch.empty((C, T, F), dtype=torch.float64, device=boxes.device)
    ob = torch.empty((C, T, F, 4), dtype=torch.float32, device=boxes.device)
    ctx.check(ctx.lib.vdet_rescore_tracks(ctx.h, tracks.contiguous().data_ptr(), ntracks.data_ptr(), boxes.data_ptr(),
                                          scores.data_ptr(), F, B, C, T, float(overlap_thres), int(window), det.data_ptr(),
                                          pooled.data_ptr(), ob.data_ptr()))
    if sync:
        ctx.sync()
    return det, pooled, ob


def track_from_anchors(boxes, anchor_frames, anchor_boxes, anchor_scores=None, link_thres=0.5, max_frames=0, sync=True,
                       ctx=None):
    """Tubelets from caller-supplied anchors: the array form of track_from_det (vdet/track.py:109-119) with the built-in
    IoU-linking tracker as ``track_method`` -- every anchor is tracked, nothing is suppressed.

    boxes [F,B,4] f32; anchor_frames [C,T] int32 (1-based, 0 = empty slot), anchor_boxes [C,T,4] f32, anchor_scores [C,T]
    f32 or None, all on the boxes' GPU.  C is only a grouping axis (C = 1: class-agnostic).  A live slot's rows are what
    ``track_volume`` makes from an anchor with that (int-truncated) box.  Returns, in ``track_volume``'s layout,
      tracks  [C,T,F,5] f32 rows (x1,y1,x2,y2,score), NaN where a tubelet has no box (an empty slot: everywhere),
      anchors [C,T,3] f32 (frame, -1, score or 0),  ntracks [C] int32 = 1 + the last live slot of the class.
    ValueError for an anchor frame outside 0..F (reported when the call, or a later ``ctx.sync()``, waits)."""
    F, B, _ = _volume_layout(boxes, nonempty=True)
    anchor_frames, anchor_boxes, anchor_scores, C, T = _anchor_slots(anchor_frames, anchor_boxes, anchor_scores)
    _same_gpu((boxes, anchor_frames, anchor_boxes, anchor_scores), "boxes, anchor_frames, anchor_boxes and anchor_scores")
    ctx = _ctx_for(boxes, ctx)
    boxes = boxes.contiguous()
    tracks, anchors, ntracks = _track_outputs(C, T, F, boxes.device, False)
    ctx.check(ctx.lib.vdet_track_from_anchors(
        ctx.h, boxes.data_ptr(), F, B, anchor_frames.data_ptr(), anchor_boxes.data_ptr(),
        anchor_scores.data_ptr() if anchor_scores is not None else None, C, T, float(link_thres), int(max_frames),
        tracks.data_ptr(), anchors.data_ptr(), ntracks.data_ptr()))
    if sync:
        ctx.sync()
    return tracks, anchors, ntracks


def _box_option(impl):
    """Gives a pixel-tracker call the two KEYWORD-ONLY options of box sampling, ``sampling='point'`` and ``integral=None``,
    behind its own parameters, whose names, order and defaults stay what they were (``inspect.signature`` reports those: it
    follows ``__wrapped__``; the two options are in the call's docstring).  With both at their defaults the decorated call runs
    as it is written; otherwise its bound arguments go to ``impl()(scale, ..., sampling=, integral=)``, the function the call
    itself ends in, with scale = (scales, scale_step, scale_penalty) where the call has them, else None."""
    def decorate(fn):
        sig = inspect.signature(fn)

        @functools.wraps(fn)
        def call(*args, sampling='point', integral=None, **kw):
            if sampling == 'point' and integral is None:
                return fn(*args, **kw)
            bound = sig.bind(*args, **kw)
            bound.apply_defaults()
            a = dict(bound.arguments)
            scale = (a.pop('scales'), a.pop('scale_step'), a.pop('scale_penalty')) if 'scales' in a else None
            return impl()(scale, sampling=sampling, integral=integral, **a)
        return call
    return decorate


def _update_option(impl):
    """Gives a pixel-tracker call the three KEYWORD-ONLY options of the template update, ``update=0``, ``update_conf=0.8`` and
    ``drift_conf=0.7``, by ``_box_option``'s mechanism and on top of it (the visible signature stays the call's own).  The
    three are checked on every call; with ``update == 0`` the call then runs as it does without them, else its bound arguments
    go to ``impl()(scale, ..., sampling=, integral=, adapt=(update, update_conf, drift_conf))``."""
    def decorate(fn):
        sig = inspect.signature(fn)

        @functools.wraps(fn)
        def call(*args, update=0, update_conf=0.8, drift_conf=0.7, sampling='point', integral=None, **kw):
            adapt = _update_settings(update, update_conf, drift_conf)
            if adapt[0] == 0:
                return fn(*args, sampling=sampling, integral=integral, **kw)
            bound = sig.bind(*args, **kw)
            bound.apply_defaults()
            a = dict(bound.arguments)
            scale = (a.pop('scales'), a.pop('scale_step'), a.pop('scale_penalty')) if 'scales' in a else None
            return impl()(scale, sampling=sampling, integral=integral, adapt=adapt, **a)
        return call
    return decorate


def _update_settings(update, update_conf, drift_conf):
    """the three checked settings of the template update"""
    update, update_conf, drift_conf = int(update), float(update_conf), float(drift_conf)
    if not 0 <= update <= 256:
        raise ValueError("update = %d; 0 .. 256" % update)
    if not math.isfinite(update_conf) or not math.isfinite(drift_conf):
        raise ValueError("update_conf and drift_conf must be finite")
    return update, update_conf, drift_conf


@_update_option(lambda: _track_pixels)
@_box_option(lambda: _track_pixels)
def track_pixels(images, anchor_frames, anchor_boxes, anchor_scores=None, grid=32, radius=8, min_conf=0.5, max_frames=0, step=1,
                 sync=True, ctx=None):
    """Tubelets that follow the PIXELS of the anchor boxes (include/vdet_hip.h: vdet_track_pixels; the rule is
    tests/pixtrack_spec.py): the array form of track_from_det with an appearance tracker as ``track_method`` -- the role of the
    reference's fcn_tracker (vdet/track.py:52-106), not its MATLAB arithmetic.  All chains of the video in one launch.

    images uint8 [F,H,W,3], contiguous, in the stored channel order (BGR from cv2.imread: never swapped); anchor_frames [C,T]
    int32 (1-based, 0 = empty slot), anchor_boxes [C,T,4] f32 (1-based inclusive), anchor_scores [C,T] f32 or None, all on the
    images' GPU: ``top_anchors``' outputs go in unchanged.  A ``grid`` x ``grid`` point-sampled luma template of the
    (int-truncated) anchor box is matched by SAD within ``radius`` grid cells on every ``step``-th frame, forward and backward;
    a chain ends when the confidence 1 - SAD / (255 * grid^2) falls below ``min_conf``, when the box leaves the image, at the
    video's end or after ceil((max_frames+1)/2) - 1 steps (max_frames = 0: no limit).  The box never changes size.
    Returns, in ``track_from_anchors``' layout,
      tracks  [C,T,F,5] f32 rows (x1,y1,x2,y2,confidence), NaN where a tubelet has no box (the frames ``step`` skips included),
      anchors [C,T,3] f32 (frame, -1, score or 0),  ntracks [C] int32 = 1 + the last live slot of the class.
    ValueError for grid not a multiple of 4 in 4..64, radius outside 1..16, step < 1, max_frames < 0 or a min_conf that is not
    finite (before any launch); and for an anchor frame outside 0..F or an anchor box that is not finite, beyond 2^20, empty or
    wholly outside the image (reported when the call, or a later ``ctx.sync()``, waits; the slot is written as an empty one).

    Keyword-only: ``sampling='box'`` (the rule's box sampling; vdet_track_pixels_box): a cell's value is the rounded mean of
    the pixels of its ``w/grid`` x ``h/grid`` rectangle instead of the one pixel at its centre, so detail finer than the pitch
    is averaged, not aliased, and motion below the pitch is followed.  The means come from ``integral``, the frames'
    ``luma_integral`` (uint32 [F,H+1,W+1], contiguous, on the images' GPU): given, the images are read for their shape only;
    None, the call builds one (two more launches).  Frames of at most 2^24 pixels.  With w == h == grid the bits are
    ``sampling='point'``'s.  ValueError (before any launch) for another ``sampling``, an integral of the wrong dtype, shape or
    device, an integral given with 'point', and H*W > 2^24 with 'box'.

    Keyword-only: ``update=0, update_conf=0.8, drift_conf=0.7``, the template update with an anchor guard (the rule is
    tests/pixtrack_adapt_spec.py; vdet_track_pixels_adaptive).  ``update`` = a in 0 .. 256 is the weight of the new patch in
    1/256; 0: the fixed template, this call as it is without the three keywords, same export, same bits.  With a > 0 every
    chain (slot AND direction; the backward chain starts from the anchor's template again) keeps A[grid,grid] in 8.8 fixed
    point, A = Tm0 << 8 at the start, and matches against Tm = (A + 128) >> 8.  After a step the chain keeps, with P the
    grid x grid window that won (on the winner's level box, before the move): c0 = 1 - sum|Tm0 - P| / (255 * grid^2) in f32;
    the update is accepted when conf >= update_conf and c0 >= drift_conf (f32 compares), and then
    A = ((256 - a) * A + a * (P << 8) + 128) >> 8 per cell.  a = 256 replaces the template every frame.  The confidence in
    column 4 is the step's, against the current template; no output is added.  An update_conf or drift_conf no step reaches
    (2.0) gives the fixed template's bits.  The guard keeps the template from absorbing something that is not the anchor's
    object.  The two default confidences are starting points that nobody has tuned on real video.  ValueError (before any
    launch) for update outside 0 .. 256 or a confidence that is not finite."""
    return _track_pixels(None, images, anchor_frames, anchor_boxes, anchor_scores, grid, radius, min_conf, max_frames, step, sync, ctx)


def _scale_settings(scales, scale_step, scale_penalty):
    """the three checked settings of the scale search"""
    scales, scale_step, scale_penalty = int(scales), int(scale_step), int(scale_penalty)
    if not 0 <= scales <= 3:
        raise ValueError("scales = %d; 0 .. 3" % scales)
    if not 1 <= scale_step <= 25:
        raise ValueError("scale_step = %d; 1 .. 25" % scale_step)
    if not 0 <= scale_penalty <= 65535:
        raise ValueError("scale_penalty = %d; 0 .. 65535" % scale_penalty)
    return scales, scale_step, scale_penalty


def _pixel_export(ctx, stem, box, scale, adapt=None):
    """The export a pixel-tracker call ends in, and the arguments it takes between the settings and the outputs: ``stem`` +
    '_box' with the scale settings (scale None: scales = 0) where ``box``, else ``stem`` itself with none (scale None) or
    ``stem`` + '_scaled' with ``scale``.  With ``adapt`` (the template update's checked settings): ``stem`` + '_adaptive', with
    the scale settings and ``adapt``; its ``box`` argument follows the planes (``_pixel_planes``)"""
    if adapt:
        return getattr(ctx.lib, stem + '_adaptive'), (scale or (0, 1, 0)) + adapt
    if box:
        return getattr(ctx.lib, stem + '_box'), scale or (0, 1, 0)
    if scale is None:
        return getattr(ctx.lib, stem), ()
    return getattr(ctx.lib, stem + '_scaled'), scale


def _pixel_planes(images, integral, box, adapt):
    """the arguments between the context and the shape: the planes a chain reads, and -- for the '_adaptive' exports -- ``box``"""
    planes = (integral.data_ptr() if box else images.data_ptr(),)
    return planes + (int(box),) if adapt else planes


def _track_pixels(scale, images, anchor_frames, anchor_boxes, anchor_scores, grid, radius, min_conf, max_frames, step, sync, ctx,
                  sampling='point', integral=None, adapt=None):
    """track_pixels (scale None) and track_pixels_scaled (scale = (scales, scale_step, scale_penalty)); with sampling='box'
    both are vdet_track_pixels_box (scale None: scales = 0); with ``adapt`` vdet_track_pixels_adaptive"""
    F, H, W = _images(images)
    box = _pixel_sampling(sampling, integral, images, F, H, W)
    anchor_frames, anchor_boxes, anchor_scores, C, T = _anchor_slots(anchor_frames, anchor_boxes, anchor_scores)
    settings = _pixel_settings(grid, radius, min_conf, max_frames, step)
    if scale is not None:
        scale = _scale_settings(*scale)
    _same_gpu((images, anchor_frames, anchor_boxes, anchor_scores, integral),
              "images, anchor_frames, anchor_boxes, anchor_scores and integral")
    ctx = _ctx_for(images, ctx)
    if box and integral is None:
        integral = luma_integral(images, sync=False, ctx=ctx)
    tracks, anchors, ntracks = _track_outputs(C, T, F, images.device, False)
    head = (ctx.h,) + _pixel_planes(images, integral, box, adapt) + (
        F, H, W, anchor_frames.data_ptr(), anchor_boxes.data_ptr(),
        anchor_scores.data_ptr() if anchor_scores is not None else None, C, T) + settings
    out = (tracks.data_ptr(), anchors.data_ptr(), ntracks.data_ptr())
    fn, extra = _pixel_export(ctx, 'vdet_track_pixels', box, scale, adapt)
    ctx.check(fn(*(head + extra + out)))
    if sync:
        ctx.sync()
    return tracks, anchors, ntracks


@_update_option(lambda: _track_pixels)
@_box_option(lambda: _track_pixels)
def track_pixels_scaled(images, anchor_frames, anchor_boxes, anchor_scores=None, grid=32, radius=8, min_conf=0.5, max_frames=0, step=1,
                        scales=1, scale_step=5, scale_penalty=0, sync=True, ctx=None):
    """``track_pixels`` with a scale search: the tubelet's box grows and shrinks with the object (include/vdet_hip.h:
    vdet_track_pixels_scaled; the rule is tests/pixtrack_spec.py's ``scales``).  On every step the current box is also tried grown and
    shrunk about its centre by ``scale_step`` percent per level, ``scales`` levels each side (0 .. 3; a side changes by
    2 * ((level * scale_step * side + 100) // 200) pixels), each level sampled on the same ``grid`` x ``grid`` cells against the
    anchor's fixed template; the smallest (SAD + level * ``scale_penalty``, level, shift) wins, the confidence is the winner's
    raw SAD's, and the winner's box, moved, is the next box.  A level whose box would have a side below 1 or above 2^21 is
    skipped.  ``scales = 0`` gives ``track_pixels``' bits.  Arguments, layouts and errors are ``track_pixels``'; in addition
    ValueError for scales outside 0..3, scale_step outside 1..25 or scale_penalty outside 0..65535 (before any launch).
    Keyword-only ``sampling`` / ``integral``: as in ``track_pixels``; every level's cells are box-filtered.
    Keyword-only ``update`` / ``update_conf`` / ``drift_conf``: the template update with an anchor guard, as in ``track_pixels``
    (vdet_track_pixels_adaptive); the patch is the winning window of the winner's level box.  The two default confidences are
    starting points that nobody has tuned on real video."""
    return _track_pixels((scales, scale_step, scale_penalty), images, anchor_frames, anchor_boxes, anchor_scores, grid, radius,
                         min_conf, max_frames, step, sync, ctx)


@_update_option(lambda: _track_volume_pixels)
@_box_option(lambda: _track_volume_pixels)
def track_volume_pixels(images, boxes, scores, nms_thres=0.3, thres=0.0, max_tracks=10, grid=32, radius=8, min_conf=0.5,
                        max_frames=0, step=1, sync=True, ctx=None):
    """Greedy tubelet generation for EVERY class of a video with the pixel tracker as ``track_method``: the array form of
    greedily_track_from_raw_dets (vdet/track.py:189-252) as ``track_volume`` is, but each anchor is followed through the PIXELS
    (``track_pixels``' rule) instead of being linked through the proposals.  Per class: the best remaining detection is the
    anchor, its tubelet is tracked, every detection the tubelet explains is removed (track_det_nms at ``nms_thres`` on the frames
    the tubelet has a box on), up to ``max_tracks`` times or until an anchor scores below ``thres``.  The rule is
    tests/pixtrack_spec.py's greedy loop; include/vdet_hip.h: vdet_track_volume_pixels.  Three launches per track, no host wait.

    images uint8 [F,H,W,3] contiguous, boxes [F,B,4] f32, scores [F,B,C] f32, all on one GPU.  Returns, in ``track_volume``'s
    layout,
      tracks  [C, max_tracks, F, 5] f32 rows (x1,y1,x2,y2,confidence; 1.0 on the anchor row), NaN where a track has no box,
      anchors [C, max_tracks, 3] f32 (1-based frame, box index, score),  ntracks [C] int32.
    ``tracks_to_proto(..., method='pixel_tracker')`` turns one class of the result into a .track dict.
    ValueError for the arguments ``track_volume`` and ``track_pixels`` refuse (before any launch); and for an anchor whose box
    is not finite, beyond 2^20, empty after truncation or wholly outside the image (reported when the call, or a later
    ``ctx.sync()``, waits): its slot is taken with NaN rows, it suppresses nothing, and the loop goes on.
    Keyword-only ``sampling`` / ``integral``: as in ``track_pixels`` (include/vdet_hip.h: vdet_track_volume_pixels_box).
    Keyword-only ``update`` / ``update_conf`` / ``drift_conf``: the template update with an anchor guard in every tubelet's
    chains, as in ``track_pixels`` (vdet_track_volume_pixels_adaptive; 0: this call as it is).  The two default confidences
    are starting points that nobody has tuned on real video."""
    return _track_volume_pixels(None, images, boxes, scores, nms_thres, thres, max_tracks, grid, radius, min_conf, max_frames, step,
                                sync, ctx)


def _track_volume_pixels(scale, images, boxes, scores, nms_thres, thres, max_tracks, grid, radius, min_conf, max_frames, step, sync,
                         ctx, sampling='point', integral=None, adapt=None):
    """track_volume_pixels (scale None) and track_volume_pixels_scaled (scale = (scales, scale_step, scale_penalty)); with
    sampling='box' both are vdet_track_volume_pixels_box (scale None: scales = 0); with ``adapt``
    vdet_track_volume_pixels_adaptive"""
    F, H, W = _images(images)
    box = _pixel_sampling(sampling, integral, images, F, H, W)
    max_tracks = int(max_tracks)
    if max_tracks < 0:
        raise ValueError("max_tracks must be >= 0")
    settings = _pixel_settings(grid, radius, min_conf, max_frames, step)
    if scale is not None:
        scale = _scale_settings(*scale)
    boxes, scores, F, B, C = _volume(boxes, scores, (images, integral), "images, integral, boxes and scores", F=F, nonempty=True)
    ctx = _ctx_for(images, ctx)
    if box and integral is None:
        integral = luma_integral(images, sync=False, ctx=ctx)
    tracks, anchors, ntracks = _track_outputs(C, max_tracks, F, images.device, True)
    head = (ctx.h,) + _pixel_planes(images, integral, box, adapt) + (
        H, W, boxes.data_ptr(), scores.data_ptr(), F, B, C, float(nms_thres), float(thres), max_tracks) + settings
    out = (tracks.data_ptr(), anchors.data_ptr(), ntracks.data_ptr())
    fn, extra = _pixel_export(ctx, 'vdet_track_volume_pixels', box, scale, adapt)
    _finish(ctx, lambda: ctx.check(fn(*(head + extra + out))), sync, reset=lambda: (tracks.fill_(float('nan')), anchors.zero_()))
    return tracks, anchors, ntracks


@_update_option(lambda: _track_volume_pixels)
@_box_option(lambda: _track_volume_pixels)
def track_volume_pixels_scaled(images, boxes, scores, nms_thres=0.3, thres=0.0, max_tracks=10, grid=32, radius=8, min_conf=0.5,
                               max_frames=0, step=1, scales=1, scale_step=5, scale_penalty=0, sync=True, ctx=None):
    """``track_volume_pixels`` with ``track_pixels_scaled``'s chain as the tracker: the tubelet that suppresses the detections it
    explains has a box that follows the object's size (include/vdet_hip.h: vdet_track_volume_pixels_scaled; the rule is the
    greedy loop of tests/pixtrack_spec.py).  ``scales = 0`` gives ``track_volume_pixels``' bits.  Arguments, layouts,
    launches and errors are ``track_volume_pixels``'; in addition ValueError for scales outside 0..3, scale_step outside 1..25
    or scale_penalty outside 0..65535 (before any launch).  Keyword-only ``sampling`` / ``integral``: as in ``track_pixels``.
    Keyword-only ``update`` / ``update_conf`` / ``drift_conf``: as in ``track_volume_pixels``
    (vdet_track_volume_pixels_adaptive); the two default confidences are starting points that nobody has tuned on real video."""
    return _track_volume_pixels((scales, scale_step, scale_penalty), images, boxes, scores, nms_thres, thres, max_tracks, grid,
                                radius, min_conf, max_frames, step, sync, ctx)


def anchor_propagate_tracks(tracks, ntracks, anchors, boxes, scores, sync=True, ctx=None):
    """anchor_propagate (vdet/tubelet_cls.py:353-383) on device tubelets: per slot, the detection of the anchor frame that
    overlaps the anchor box most (f64 ``iou``, ``np.argmax``: first maximum, a NaN overlap counts as the maximum) lends its
    class score to every box of the tubelet.

    tracks [C,T,F,5] f32 / ntracks [C] int32 / anchors [C,T,3] f32 (track_from_anchors, track_volume, nms_track_volume),
    boxes [F,B,4] f32, scores [F,B,C] f32.  Returns (det_score [C,T,F] f64: the score where the tubelet has a box, NaN
    elsewhere; best [C,T] int32: the detection's index on the anchor frame, -1 for a slot without anchor box)."""
    C, T, F = _tubelets_layout(tracks, ntracks, anchors)
    boxes, scores, F, B, C = _volume(boxes, scores, (tracks, ntracks, anchors), "tracks, ntracks, anchors, boxes and scores",
                                     F=F, C=C, nonempty=True)
    ctx = _ctx_for(boxes, ctx)
    det = torch.empty((C, T, F), dtype=torch.float64, device=boxes.device)
    best = torch.empty((C, T), dtype=torch.int32, device=boxes.device)
    ctx.check(ctx.lib.vdet_anchor_propagate_tracks(
        ctx.h, tracks.contiguous().data_ptr(), ntracks.contiguous().data_ptr(), anchors.contiguous().data_ptr(),
        boxes.data_ptr(), scores.data_ptr(), F, B, C, T, det.data_ptr(), best.data_ptr()))
    if sync:
        ctx.sync()
    return det, best


def top_anchors(boxes, scores, top_num, mode='video', score_thresh=None, frame_off=None, sync=True, ctx=None):
    """The array form of protocol.top_detections (mode='video', utils/protocol.py:330-339) and frame_top_detections
    (mode='frame', :341-351) for EVERY class in one call: the anchors ``track_from_anchors`` takes.

    boxes [F,B,4] f32, scores [F,B,C] f32 (class innermost), same GPU.  A candidate of class c is a detection whose score is
    not NaN and -- with ``score_thresh`` -- is > score_thresh (float32 compare, as ``nms_volume``; ``-inf`` drops io.py's
    padding; without a threshold ``-inf`` IS a candidate: it is what ``det_score`` returns for a missing class).  Candidates
    are ordered by descending score, equal scores (-0.0 == +0.0) by ascending flat index f*B + b, like Python's stable
    ``sorted(..., reverse=True)`` over a frame-major det_proto.  One point of the reference is NOT mirrored: it returns a
    proto of fewer than ``top_num`` detections unsorted; this call always sorts.
      mode='video': T = top_num (<= 1024); slot t of class c is the t-th candidate; slots behind the last one are empty.
        With ``frame_off`` [V+1] the selection runs inside every video's frame range, the outputs are [V,C,T,...] and frames
        are local to the video (``track_from_anchors_batch``'s inputs).
      mode='frame': T = F*top_num (top_num <= 128); slot f*top_num + r is the r-th candidate of frame f (frames ascending).
        No batch form (ValueError with ``frame_off``).
    Returns anchor_frames [C,T] int32 (1-based, 0 = empty slot), anchor_boxes [C,T,4] f32 (the proposal's box, not
    truncated), anchor_scores [C,T] f32, anchor_index [C,T] int32 (box index in its frame, -1 = empty); an empty slot's box
    and score are 0."""
    if mode not in ('video', 'frame'):
        raise ValueError("mode must be 'video' or 'frame'")
    if mode == 'frame' and frame_off is not None:
        raise ValueError("mode='frame' has no batch form (frame_off)")
    top_num = int(top_num)
    if top_num < 1:
        raise ValueError("top_num must be at least 1")
    if top_num > (1024 if mode == 'video' else 128):
        raise ValueError("top_num is limited to 1024 (mode='video') / 128 (mode='frame')")
    F, B, C = _volume_layout(boxes, scores, nonempty=True)
    off = None if frame_off is None else _frame_offsets(frame_off, F)
    _same_gpu((boxes, scores), "boxes and scores")
    ctx = _ctx_for(boxes, ctx)
    boxes, scores = boxes.contiguous(), scores.contiguous()
    T = top_num if mode == 'video' else F * top_num
    lead = (C, T) if off is None else (len(off) - 1, C, T)
    dev = boxes.device
    frames = torch.empty(lead, dtype=torch.int32, device=dev)
    aboxes = torch.empty(lead + (4,), dtype=torch.float32, device=dev)
    ascores = torch.empty(lead, dtype=torch.float32, device=dev)
    index = torch.empty(lead, dtype=torch.int32, device=dev)
    ctx.check(ctx.lib.vdet_top_anchors(
        ctx.h, boxes.data_ptr(), scores.data_ptr(), F, B, C, top_num, 0 if mode == 'video' else 1,
        0 if score_thresh is None else 1, 0.0 if score_thresh is None else float(score_thresh),
        off.ctypes.data if off is not None else None, 0 if off is None else len(off) - 1,
        frames.data_ptr(), aboxes.data_ptr(), ascores.data_ptr(), index.data_ptr()))
    if sync:
        ctx.sync()
    return frames, aboxes, ascores, index


def track_from_anchors_batch(boxes, frame_off, anchor_frames, anchor_boxes, anchor_scores=None, link_thres=0.5, max_frames=0,
                             sync=True, ctx=None):
    """``track_from_anchors`` for V videos in ONE launch.  boxes [F,B,4] f32 holds the videos' frames one after the other,
    ``frame_off`` [V+1] their ranges; anchor_frames [V,C,T] int32 (1-based INSIDE the video, 0 = empty slot), anchor_boxes
    [V,C,T,4] f32, anchor_scores [V,C,T] f32 or None (``top_anchors(frame_off=...)``'s outputs).  A chain stops at its own
    video's first and last frame; per video the rows are bit for bit ``track_from_anchors``' on that video alone.
    Returns a dict in ``video_batch``'s layout (``_batch_read``): tracks, anchors, ntracks, frame_off.  ValueError for an anchor
    frame outside 0..F_v."""
    F, B, _ = _volume_layout(boxes, nonempty=True)
    off = _frame_offsets(frame_off, F)
    V = len(off) - 1
    anchor_frames, anchor_boxes, anchor_scores, C, T = _anchor_slots(anchor_frames, anchor_boxes, anchor_scores, V)
    _same_gpu((boxes, anchor_frames, anchor_boxes, anchor_scores), "boxes, anchor_frames, anchor_boxes and anchor_scores")
    ctx = _ctx_for(boxes, ctx)
    boxes = boxes.contiguous()
    tracks, anchors, ntracks = _track_outputs(C, T, F, boxes.device, False, V=V)
    ctx.check(ctx.lib.vdet_track_from_anchors_batch(
        ctx.h, boxes.data_ptr(), off.ctypes.data, V, B, anchor_frames.data_ptr(), anchor_boxes.data_ptr(),
        anchor_scores.data_ptr() if anchor_scores is not None else None, C, T, float(link_thres), int(max_frames),
        tracks.data_ptr(), anchors.data_ptr(), ntracks.data_ptr()))
    if sync:
        ctx.sync()
    return dict(tracks=_batch_views(tracks, off, C, T, 5), anchors=anchors, ntracks=ntracks, frame_off=off)


def anchor_propagate_tracks_batch(batch_out, boxes, scores, sync=True, ctx=None):
    """``anchor_propagate_tracks`` for every video of a ``track_from_anchors_batch`` (or ``video_batch``) result in ONE
    launch; boxes [F,B,4] / scores [F,B,C] f32 are the batch's volume.  Returns (det, best): det, the [C,T,F_v] f64 views of
    the batch layout (``_batch_read``) -- also stored as ``batch_out['det']``, where ``tcn_tracks_batch(series='det')`` reads
    it -- and best [V,C,T] int32.  Per video both equal the single-video call's."""
    b = _batch_read(batch_out, need=('anchors',))
    off, V, F, C, T, tracks, ntracks, anchors = b.off, b.V, b.Ft, b.C, b.T, b.tracks, b.ntracks, b.anchors
    boxes, scores, F, B, C = _volume(boxes, scores, (tracks, ntracks, anchors), "the batch result, boxes and scores", F=F, C=C)
    ctx = _ctx_for(boxes, ctx)
    dev = boxes.device
    det = torch.empty((C * T * F,), dtype=torch.float64, device=dev)
    best = torch.empty((V, C, T), dtype=torch.int32, device=dev)
    ctx.check(ctx.lib.vdet_anchor_propagate_tracks_batch(
        ctx.h, tracks.data_ptr(), ntracks.data_ptr(), anchors.data_ptr(), boxes.data_ptr(), scores.data_ptr(), off.ctypes.data,
        V, B, C, T, det.data_ptr(), best.data_ptr()))
    if sync:
        ctx.sync()
    dv = _batch_views(det, off, C, T, 1)
    batch_out['det'] = dv
    return dv, best


def _tcn_net_args(net):
    from .vdet.tcn import TCNNet
    if not isinstance(net, TCNNet):
        raise ValueError("net must be a vdetlib_amd.vdet.tcn.TCNNet")
    params, shapes = net.packed()
    codes = net.device_channels()
    return params, shapes, codes


def _tcn_check(tracks, ntracks, anchors, det_score, gt_overlap, V, C, T, n, codes):
    """Shared validation of tcn_tracks / tcn_tracks_batch: flat element counts ``n`` = C*T*F_total."""
    if tracks.dtype != torch.float32 or tracks.numel() != n * 5:
        raise ValueError("tracks must be float32 [C,T,F,5]")
    if ntracks.dtype != torch.int32 or ntracks.numel() != V * C:
        raise ValueError("ntracks must be int32 [C] (batch: [V,C])")
    if anchors.dtype != torch.float32 or anchors.numel() != V * C * T * 3:
        raise ValueError("anchors must be float32 [C,T,3] (batch: [V,C,T,3])")
    if det_score.dtype not in (torch.float32, torch.float64) or det_score.numel() != n:
        raise ValueError("det_score must be float32 / float64 [C,T,F]")
    if gt_overlap is not None and (gt_overlap.dtype != torch.float64 or gt_overlap.numel() != n):
        raise ValueError("gt_overlap must be float64 [C,T,F]")
    if gt_overlap is None and any(int(q) in (4, 5) for q in codes):
        raise ValueError("the net reads gt_overlaps / labels: pass gt_overlap (ops.tubelets_overlap)")
    every = (tracks, ntracks, anchors, det_score) + (() if gt_overlap is None else (gt_overlap,))
    if not all(t.is_contiguous() for t in every):
        raise ValueError("tensors must be contiguous")
    _same_gpu(every, "tracks, ntracks, anchors, det_score and gt_overlap")


_TCN_ROW_DTYPES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2, torch.float64: 3}      # include/vdet_hip.h


def _tcn_wide_args(net, wide, rows_of, device):
    """The per-input host tables of vdet_tcn_tracks_wide[_batch] for ``net`` and the ``wide`` dict (blob name -> rows):
    (params, shapes, codes of the one-channel inputs, (codes, widths, row pointers, dtypes) int32 / uint64 arrays, the row
    tensors to keep alive).  ``rows_of(name, rows, ch)`` returns the checked flat tensor of one blob."""
    from .vdet.tcn import TCNNet
    if not isinstance(net, TCNNet):
        raise ValueError("net must be a vdetlib_amd.vdet.tcn.TCNNet")
    params, shapes = net.packed()
    inputs = net.device_inputs(wide)
    n = len(inputs)
    codes, widths = np.zeros(n, np.int32), np.zeros(n, np.int32)
    ptrs, dtypes = np.zeros(n, np.uint64), np.zeros(n, np.int32)
    keep = []
    for i, ((name, _), (code, ch)) in enumerate(zip(net.inputs, inputs)):
        codes[i], widths[i] = code, ch
        if code != -1:
            continue
        rows = rows_of(name, wide[name], ch)
        if rows.dtype not in _TCN_ROW_DTYPES:
            raise ValueError("wide rows must be float32 / float16 / bfloat16 / float64; %r is %s" % (name, rows.dtype))
        if not rows.is_contiguous():
            raise ValueError("wide rows must be contiguous; %r is not" % name)
        _same_gpu((rows,), "tracks and the wide rows %r" % name, device)
        ptrs[i], dtypes[i] = rows.data_ptr(), _TCN_ROW_DTYPES[rows.dtype]
        keep.append(rows)
    return params, shapes, codes[codes >= 0].copy(), (codes, widths, ptrs, dtypes), keep


def tcn_tracks(net, tracks, ntracks, anchors, det_score, gt_overlap=None, sync=True, ctx=None, wide=None):
    """The tubelet temporal-convolution scorer (score_conv_cls, vdet/tubelet_cls.py:15-51) on device tubelets: channel
    assembly and every layer of ``net`` (a ``vdet.tcn.TCNNet`` whose inputs are one-channel blobs among det_scores,
    track_scores, anchors, abs_anchors, gt_overlaps, labels) in two launches for ALL tubelets of the video.

    tracks [C,T,F,5] f32 / ntracks [C] int32 / anchors [C,T,3] f32 (track_volume, nms_track_volume), det_score [C,T,F] f64
    or f32 (rescore_tracks' det_score or pooled), gt_overlap [C,T,F] f64 (tubelets_overlap) when the net reads it.
    Returns conv_score [C,T,F] f32: probs[1] per box, NaN where there is none -- bit for bit what ``score_conv_cls`` writes
    on the protocol dicts of the same tensors; feeds ``DetEvaluator.add_tracks(..., scores=conv_score)`` as is.

    ``wide``: dict blob name -> rows [C,T,F,W] (f32 / f16 / bf16 / f64, contiguous, on the tracks' GPU) for the net's WIDE
    blobs, e.g. ``{'all_scores': ..., 'feats': ...}``: channel q of the blob at series position j is entry q of the row of
    the tubelet's j-th box; W must equal the blob's channel count.  Rows of holes and of slots behind ntracks are never
    read.  The first layer then runs in a kernel of its own that reads the rows where they lie (three launches in all);
    results stay bit-equal to ``TCNNet.forward`` on the same [Cin, L] input.  Without ``wide`` the call is the narrow one."""
    if wide:
        return _tcn_tracks_wide(net, tracks, ntracks, anchors, det_score, gt_overlap, sync, ctx, wide)
    params, shapes, codes = _tcn_net_args(net)
    if tracks.dim() != 4 or tracks.shape[3] != 5:
        raise ValueError("tracks must be float32 [C,T,F,5]")
    C, T, F = tracks.shape[0], tracks.shape[1], tracks.shape[2]
    if tuple(ntracks.shape) != (C,) or tuple(anchors.shape) != (C, T, 3) or tuple(det_score.shape) != (C, T, F) or \
            (gt_overlap is not None and tuple(gt_overlap.shape) != (C, T, F)):
        raise ValueError("ntracks [C], anchors [C,T,3], det_score / gt_overlap [C,T,F]")
    if F < 1:
        raise ValueError("a video needs at least one frame")
    tracks, ntracks, anchors, det_score = tracks.contiguous(), ntracks.contiguous(), anchors.contiguous(), det_score.contiguous()
    gt_overlap = None if gt_overlap is None else gt_overlap.contiguous()
    _tcn_check(tracks, ntracks, anchors, det_score, gt_overlap, 1, C, T, C * T * F, codes)
    ctx = _ctx_for(tracks, ctx)
    out = torch.empty((C, T, F), dtype=torch.float32, device=tracks.device)
    ctx.check(ctx.lib.vdet_tcn_tracks(
        ctx.h, params.ctypes.data, shapes.ctypes.data, len(net.layers), codes.ctypes.data, len(codes), F, C, T, tracks.data_ptr(),
        ntracks.data_ptr(), anchors.data_ptr(), det_score.data_ptr(), int(det_score.dtype == torch.float64),
        gt_overlap.data_ptr() if gt_overlap is not None else None, out.data_ptr()))
    if sync:
        ctx.sync()
    return out


def _tcn_tracks_wide(net, tracks, ntracks, anchors, det_score, gt_overlap, sync, ctx, wide):
    """``tcn_tracks`` with wide blobs (vdet_tcn_tracks_wide)."""
    if not isinstance(wide, dict):
        raise ValueError("wide must be a dict: blob name -> rows [C,T,F,W]")
    if tracks.dim() != 4 or tracks.shape[3] != 5:
        raise ValueError("tracks must be float32 [C,T,F,5]")
    C, T, F = tracks.shape[0], tracks.shape[1], tracks.shape[2]

    def rows_of(name, rows, ch):
        if not isinstance(rows, torch.Tensor) or tuple(rows.shape) != (C, T, F, ch):
            raise ValueError("wide[%r] must be a tensor [C,T,F,%d]: the blob's channel count is the rows' width" % (name, ch))
        return rows

    params, shapes, codes, (wcodes, widths, ptrs, dtypes), keep = _tcn_wide_args(net, wide, rows_of, tracks.device)
    if tuple(ntracks.shape) != (C,) or tuple(anchors.shape) != (C, T, 3) or tuple(det_score.shape) != (C, T, F) or \
            (gt_overlap is not None and tuple(gt_overlap.shape) != (C, T, F)):
        raise ValueError("ntracks [C], anchors [C,T,3], det_score / gt_overlap [C,T,F]")
    if F < 1:
        raise ValueError("a video needs at least one frame")
    tracks, ntracks, anchors, det_score = tracks.contiguous(), ntracks.contiguous(), anchors.contiguous(), det_score.contiguous()
    gt_overlap = None if gt_overlap is None else gt_overlap.contiguous()
    _tcn_check(tracks, ntracks, anchors, det_score, gt_overlap, 1, C, T, C * T * F, codes)
    ctx = _ctx_for(tracks, ctx)
    out = torch.empty((C, T, F), dtype=torch.float32, device=tracks.device)
    ctx.check(ctx.lib.vdet_tcn_tracks_wide(
        ctx.h, params.ctypes.data, shapes.ctypes.data, len(net.layers), wcodes.ctypes.data, widths.ctypes.data, ptrs.ctypes.data,
        dtypes.ctypes.data, len(wcodes), F, C, T, tracks.data_ptr(), ntracks.data_ptr(), anchors.data_ptr(), det_score.data_ptr(),
        int(det_score.dtype == torch.float64), gt_overlap.data_ptr() if gt_overlap is not None else None, out.data_ptr()))
    if sync:
        ctx.sync()
    return out


def tcn_tracks_batch(net, batch_out, series='det', gt_overlap=None, sync=True, ctx=None, wide=None):
    """``tcn_tracks`` for every video of a dict in ``video_batch``'s layout (``_batch_read``) in ONE assembly launch and ONE
    network launch.  ``series``: which re-scored series feeds det_scores ('det' or 'pooled'); gt_overlap: the flat f64 buffer
    ``tubelets_overlap_batch`` returns.  Returns the list of per-video conv_score [C,T,F_v] f32 views.
    ``wide``: as in ``tcn_tracks``, in the batch layout: per blob one flat tensor [C*T*F_total, W], or the list of its
    per-video views [C,T,F_v,W], checked like every field of the layout."""
    b = _batch_read(batch_out, need=('anchors',))
    off, V, Ft, C, T, tracks, ntracks, anchors = b.off, b.V, b.Ft, b.C, b.T, b.tracks, b.ntracks, b.anchors
    if series not in ('det', 'pooled') or not batch_out.get(series):
        raise ValueError("series must be 'det' or 'pooled' of a video_batch result that ran the re-scoring")
    det = _batch_field(b, batch_out[series], 1, _F32_F64, series, 'batch_out')
    if wide:
        if not isinstance(wide, dict):
            raise ValueError("wide must be a dict: blob name -> rows")

        def rows_of(name, rows, ch):
            if isinstance(rows, (list, tuple)):
                return _batch_field(b, rows, ch, tuple(_TCN_ROW_DTYPES), "wide[%r]" % name, 'tcn_tracks_batch',
                                    axis=True).view(C * T * Ft, ch)
            if not isinstance(rows, torch.Tensor) or tuple(rows.shape) != (C * T * Ft, ch):
                raise ValueError("wide[%r] must be a tensor [C*T*F_total,%d] or its per-video views: the blob's channel count is "
                                 "the rows' width" % (name, ch))
            return rows

        params, shapes, codes, wargs, _keep = _tcn_wide_args(net, wide, rows_of, b.device)
    else:
        params, shapes, codes = _tcn_net_args(net)
        wargs = None
    _tcn_check(tracks, ntracks, anchors, det, gt_overlap, V, C, T, C * T * Ft, codes)
    ctx = _ctx_for(tracks, ctx)
    out = torch.empty((C * T * Ft,), dtype=torch.float32, device=tracks.device)
    if wargs is not None:
        wcodes, widths, ptrs, dtypes = wargs
        ctx.check(ctx.lib.vdet_tcn_tracks_wide_batch(
            ctx.h, params.ctypes.data, shapes.ctypes.data, len(net.layers), wcodes.ctypes.data, widths.ctypes.data,
            ptrs.ctypes.data, dtypes.ctypes.data, len(wcodes), off.ctypes.data, V, C, T, tracks.data_ptr(), ntracks.data_ptr(),
            anchors.data_ptr(), det.data_ptr(), int(det.dtype == torch.float64),
            gt_overlap.data_ptr() if gt_overlap is not None else None, out.data_ptr()))
    else:
        ctx.check(ctx.lib.vdet_tcn_tracks_batch(
            ctx.h, params.ctypes.data, shapes.ctypes.data, len(net.layers), codes.ctypes.data, len(codes), off.ctypes.data, V, C, T,
            tracks.data_ptr(), ntracks.data_ptr(), anchors.data_ptr(), det.data_ptr(), int(det.dtype == torch.float64),
            gt_overlap.data_ptr() if gt_overlap is not None else None, out.data_ptr()))
    if sync:
        ctx.sync()
    return _batch_views(out, off, C, T, 1)


def _interp_frames(frames, off, num_frames):
    """The host tables of interpolate_tracks[_batch]: frames (flat int32, or None: identity) and the dense frame counts
    [V], checked per video against the sampled offsets ``off``."""
    V = len(off) - 1
    nf = np.ascontiguousarray(num_frames, dtype=np.int64).reshape(-1)
    if nf.size != V:
        raise ValueError("num_frames: one dense frame count per video")
    if frames is None:
        if np.any(nf < np.diff(off)):
            raise ValueError("num_frames must not be smaller than the number of rows when frames is None")
        return None, nf
    fr = np.asarray(frames.cpu() if hasattr(frames, 'cpu') else frames)
    if fr.dtype.kind not in 'iu' or fr.ndim != 1:
        raise ValueError("frames must be a 1-D integer array of dense 1-based frame numbers")
    if fr.size != int(off[-1]):
        raise ValueError("frames must name the dense frame of every row (%d rows, %d frames)" % (int(off[-1]), fr.size))
    fr = fr.astype(np.int64)
    if np.any(fr[off[:-1]] < 1):
        raise ValueError("frames are 1-based: the first frame of a video must be >= 1")
    inner = np.ones(max(fr.size - 1, 0), dtype=bool)
    inner[off[1:-1] - 1] = False                      # the step from one video's last row to the next one's first
    if np.any((np.diff(fr) <= 0) & inner):
        raise ValueError("frames must be strictly ascending inside a video")
    if np.any(nf < fr[off[1:] - 1]):
        raise ValueError("num_frames is smaller than the last frame of a video")
    return np.ascontiguousarray(fr, dtype=np.int32), nf


def _interp_series(series, n, device):
    if torch.is_tensor(series):
        series = (series,)
    series = tuple(series)
    if len(series) > 4:
        raise ValueError("at most 4 series per call")
    for x in series:
        if not torch.is_tensor(x) or x.dtype not in (torch.float32, torch.float64) or x.numel() != n:
            raise ValueError("every series must be a float32 / float64 tensor [C,T,Fs]")
        if x.dtype != series[0].dtype:
            raise ValueError("the series of one call must share one dtype")
    _same_gpu(series, "tracks, ntracks, anchors, boxes and the series", device)
    return tuple(x.contiguous() for x in series)


def _interp_call(ctx, single, soff, doff, fr, C, T, tracks, boxes, ntracks, anchors, series, sync):
    """Allocate the dense outputs (flat, batch layout) and enqueue the one launch."""
    dev = tracks.device
    V, N = len(doff) - 1, C * T * int(doff[-1])
    if N >= 2 ** 31 - 16 or C * T * int(soff[-1]) >= 2 ** 31 - 16:
        raise ValueError("too many tubelet boxes (C*T*F must stay below 2^31)")
    out_tr = torch.empty((N * 5,), dtype=torch.float32, device=dev)
    b64 = torch.empty((N * 4,), dtype=torch.float64, device=dev)
    tb = torch.empty((N * 4,), dtype=torch.float32, device=dev)
    ser = torch.empty((len(series), N), dtype=torch.float64, device=dev)
    anchor = torch.empty((N,), dtype=torch.float64, device=dev)
    oan = torch.empty((V, C, T, 3), dtype=torch.float32, device=dev)
    ptrs = (ctypes.c_void_p * 4)(*[x.data_ptr() for x in series])
    f64 = int(bool(series) and series[0].dtype == torch.float64)
    tail = (C, T, tracks.data_ptr(), boxes.data_ptr() if boxes is not None else None, ntracks.data_ptr(), anchors.data_ptr(), ptrs,
            len(series), f64, out_tr.data_ptr(), b64.data_ptr(), tb.data_ptr(), ser.data_ptr(), anchor.data_ptr(), oan.data_ptr())
    frp = fr.ctypes.data if fr is not None else None
    if single:
        ctx.check(ctx.lib.vdet_interp_tracks(ctx.h, int(soff[-1]), int(doff[-1]), frp, *tail))
    else:
        ctx.check(ctx.lib.vdet_interp_tracks_batch(ctx.h, soff.ctypes.data, doff.ctypes.data, V, frp, *tail))
    if sync:
        ctx.sync()
    return out_tr, b64, tb, ser, anchor, oan


def interpolate_tracks(tracks, ntracks, anchors, series, boxes=None, frames=None, num_frames=None, sync=True, ctx=None):
    """``score_proto_interpolation`` (vdet/tubelet_cls.py:416-490) on device tubelets: tubelets tracked and re-scored on
    every stride-th frame (``nms_track_volume`` / ``rescore_tracks`` on ``boxes[::stride]``, ``scores[::stride]``), or
    tubelets with holes (NaN rows), back to EVERY frame of the video -- all tubelets in one launch, no host wait.

    tracks [C,T,Fs,5] f32 / ntracks [C] int32 / anchors [C,T,3] f32 on the sampled axis; row i is the dense 1-based frame
    ``frames[i]`` (strictly ascending ints; None: i + 1, the axis is dense already and only holes are filled);
    ``num_frames`` = F, the frames of the dense video (default: the last of ``frames``, else Fs).  ``series``: up to 4
    tensors [C,T,Fs], all f64 or all f32 (rescore_tracks' det_score / pooled, a conv_score ...); ``boxes`` [C,T,Fs,4] f32
    to interpolate instead of the track boxes (rescore_tracks' boxes).  Semantics per tubelet, arithmetic and the end rule:
    include/vdet_hip.h (vdet_interp_tracks) -- bit for bit oracle.tubelet_interpolation on the same numbers.

    Returns a dict: ``tracks`` [C,T,F,5] f32 (interpolated box and track score, each rounded once from f64; NaN rows where
    the tubelet has no dense box), ``boxes64`` [C,T,F,4] f64, ``tboxes`` [C,T,F,4] f32 (boxes64 rounded once), ``series``
    (tuple of [C,T,F] f64), ``anchor`` [C,T,F] f64 (offset from the anchor in dense frames), ``anchors`` [C,T,3] f32
    (column 0 = the anchor's dense frame number), ``ntracks``.  The track score is interpolated like a score (the
    reference's interpolated boxes have none: build-defined)."""
    if not torch.is_tensor(tracks) or tracks.dtype != torch.float32 or tracks.dim() != 4 or tracks.shape[3] != 5:
        raise ValueError("tracks must be float32 [C,T,Fs,5]")
    C, T, Fs = tracks.shape[0], tracks.shape[1], tracks.shape[2]
    if Fs < 1 or C < 1:
        raise ValueError("a video needs at least one frame and one class")
    if ntracks.dtype != torch.int32 or tuple(ntracks.shape) != (C,):
        raise ValueError("ntracks must be int32 [C]")
    if anchors.dtype != torch.float32 or tuple(anchors.shape) != (C, T, 3):
        raise ValueError("anchors must be float32 [C,T,3]")
    if boxes is not None and (boxes.dtype != torch.float32 or tuple(boxes.shape) != (C, T, Fs, 4)):
        raise ValueError("boxes must be float32 [C,T,Fs,4]")
    _same_gpu((tracks, ntracks, anchors, boxes), "tracks, ntracks, anchors, boxes and the series")
    series = _interp_series(series, C * T * Fs, tracks.device)
    for x in series:
        if tuple(x.shape) != (C, T, Fs):
            raise ValueError("every series must be a float32 / float64 tensor [C,T,Fs]")
    soff = np.array([0, Fs], dtype=np.int64)
    if num_frames is None:
        last = np.asarray(frames.cpu() if hasattr(frames, 'cpu') else frames).reshape(-1)[-1:] if frames is not None else []
        num_frames = int(last[0]) if len(last) else Fs
    fr, nf = _interp_frames(frames, soff, [int(num_frames)])
    doff = np.array([0, int(nf[0])], dtype=np.int64)
    tracks, ntracks, anchors = tracks.contiguous(), ntracks.contiguous(), anchors.contiguous()
    boxes = None if boxes is None else boxes.contiguous()
    ctx = _ctx_for(tracks, ctx)
    out_tr, b64, tb, ser, anchor, oan = _interp_call(ctx, True, soff, doff, fr, C, T, tracks, boxes, ntracks, anchors, series, sync)
    F = int(nf[0])
    return dict(tracks=out_tr.view(C, T, F, 5), boxes64=b64.view(C, T, F, 4), tboxes=tb.view(C, T, F, 4),
                series=tuple(ser[q].view(C, T, F) for q in range(len(series))), anchor=anchor.view(C, T, F),
                anchors=oan.view(C, T, 3), ntracks=ntracks)


def interpolate_tracks_batch(batch_out, frames, num_frames, sync=True, ctx=None):
    """``interpolate_tracks`` for every video of a ``video_batch`` result that was computed on SAMPLED frames, in one
    launch: ``frames`` flat [Fs_total] ints (the dense 1-based frame of every row, ascending inside each video; None:
    identity), ``num_frames`` [V] the dense frame counts.  The re-scored ``det`` / ``pooled`` series and ``tboxes`` are
    interpolated when the batch has them (else the track boxes, no series).  Returns a dict in the same layout
    (``_batch_read``) on the DENSE axis -- ``tracks``, ``det`` / ``pooled`` / ``tboxes`` (empty lists without re-scoring),
    ``anchors``, ``ntracks``, the dense ``frame_off`` -- plus ``boxes64`` and ``anchor`` views."""
    b = _batch_read(batch_out, need=('anchors',))
    soff, V, Fs, C, T, tracks, ntracks, anchors = b.off, b.V, b.Ft, b.C, b.T, b.tracks, b.ntracks, b.anchors
    rescored = bool(batch_out.get('pooled'))
    field = lambda k, per, dtypes: _batch_field(b, batch_out.get(k), per, dtypes, k, 'batch_out')
    series = (field('det', 1, _F32_F64), field('pooled', 1, _F32_F64)) if rescored else ()
    boxes = field('tboxes', 4, _F32) if rescored else None
    series = _interp_series(series, C * T * Fs, b.device)
    _same_gpu((tracks, ntracks, anchors, boxes), "tracks, ntracks, anchors, boxes and the series")
    fr, nf = _interp_frames(frames, soff, num_frames)
    doff = np.concatenate([[0], np.cumsum(nf)]).astype(np.int64)
    ctx = _ctx_for(tracks, ctx)
    out_tr, b64, tb, ser, anchor, oan = _interp_call(ctx, False, soff, doff, fr, C, T, tracks, boxes, ntracks, anchors, series, sync)
    views = lambda flat, per: _batch_views(flat, doff, C, T, per)
    out = dict(tracks=views(out_tr, 5), tboxes=views(tb, 4), boxes64=views(b64, 4), anchor=views(anchor, 1), anchors=oan,
               ntracks=ntracks, frame_off=doff, det=[], pooled=[])
    if rescored:
        out.update(det=views(ser[0], 1), pooled=views(ser[1], 1))
    return out


_MERGE_SCHEMES = {'combine': 0, 'max': 1}      # include/vdet_hip.h: VDET_MERGE_COMBINE / VDET_MERGE_MAX


def _merge_series(series, shape, who):
    if torch.is_tensor(series):
        series = (series,)
    series = tuple(series)
    if not 1 <= len(series) <= 4:
        raise ValueError("%s: 1 to 4 series (series 0 is det_score)" % who)
    for x in series:
        if not torch.is_tensor(x) or x.dtype != torch.float64 or tuple(x.shape) != shape:
            raise ValueError("%s: every series must be a float64 tensor [C,T,F]" % who)
    return series


def _merge_set(s, who):
    """One side of merge_tracks, checked: (tracks, ntracks, anchors, tboxes or None, series tuple)."""
    if not isinstance(s, dict) or any(k not in s for k in ('tracks', 'ntracks', 'anchors', 'series')):
        raise ValueError("%s must be a dict with tracks, ntracks, anchors and series (optionally tboxes)" % who)
    tracks, ntracks, anchors, tboxes = s['tracks'], s['ntracks'], s['anchors'], s.get('tboxes')
    if not torch.is_tensor(tracks) or tracks.dtype != torch.float32 or tracks.dim() != 4 or tracks.shape[3] != 5:
        raise ValueError("%s: tracks must be float32 [C,T,F,5]" % who)
    C, T, F = tracks.shape[0], tracks.shape[1], tracks.shape[2]
    if C < 1 or F < 1:
        raise ValueError("%s: at least one class and one frame" % who)
    if not torch.is_tensor(ntracks) or ntracks.dtype != torch.int32 or tuple(ntracks.shape) != (C,):
        raise ValueError("%s: ntracks must be int32 [C]" % who)
    if not torch.is_tensor(anchors) or anchors.dtype != torch.float32 or tuple(anchors.shape) != (C, T, 3):
        raise ValueError("%s: anchors must be float32 [C,T,3]" % who)
    if tboxes is not None and (not torch.is_tensor(tboxes) or tboxes.dtype != torch.float32 or tuple(tboxes.shape) != (C, T, F, 4)):
        raise ValueError("%s: tboxes must be float32 [C,T,F,4]" % who)
    return tracks, ntracks, anchors, tboxes, _merge_series(s['series'], (C, T, F), who)


def _merge_call(ctx, scheme, off, C, Ta, Tb, sa, sb, sync):
    """Allocate the outputs (flat, batch layout) and enqueue the one launch.  sa / sb: (tracks, ntracks, anchors, tboxes or
    None, series tuple), contiguous, one device.  Returns (tracks, ntracks, anchors, tboxes or None, series [n, N], from_b or
    None, T_out), all flat."""
    V, Ft = len(off) - 1, int(off[-1])
    To = Ta + Tb if scheme == 'combine' else Ta
    if max(C * To * Ft, C * Tb * Ft, V * C * max(To, Tb)) >= 2 ** 31 - 16:
        raise ValueError("too many tubelet boxes (C*T*F must stay below 2^31 - 16, the output's T included)")
    dev = sa[0].device
    n, N = len(sa[4]), C * To * Ft
    tracks = torch.empty((N * 5,), dtype=torch.float32, device=dev)
    ntracks = torch.empty((V, C), dtype=torch.int32, device=dev)
    anchors = torch.empty((V, C, To, 3), dtype=torch.float32, device=dev)
    tboxes = torch.empty((N * 4,), dtype=torch.float32, device=dev) if sa[3] is not None else None
    series = torch.empty((n, N), dtype=torch.float64, device=dev)
    from_b = torch.empty((N,), dtype=torch.uint8, device=dev) if scheme == 'max' else None
    pa = (ctypes.c_void_p * 4)(*[x.data_ptr() for x in sa[4]])
    pb = (ctypes.c_void_p * 4)(*[x.data_ptr() for x in sb[4]])
    ptr = lambda x: x.data_ptr() if x is not None else None
    tail = (C, Ta, Tb, sa[0].data_ptr(), sa[1].data_ptr(), sa[2].data_ptr(), ptr(sa[3]), sb[0].data_ptr(), sb[1].data_ptr(),
            sb[2].data_ptr(), ptr(sb[3]), pa, pb, n, tracks.data_ptr(), ntracks.data_ptr(), anchors.data_ptr(), ptr(tboxes),
            series.data_ptr(), ptr(from_b))
    if V == 1:
        ctx.check(ctx.lib.vdet_merge_tracks(ctx.h, _MERGE_SCHEMES[scheme], Ft, *tail))
    else:
        ctx.check(ctx.lib.vdet_merge_tracks_batch(ctx.h, _MERGE_SCHEMES[scheme], off.ctypes.data, V, *tail))
    if sync:
        ctx.sync()
    return tracks, ntracks, anchors, tboxes, series, from_b, To


def merge_tracks(a, b, scheme='combine', sync=True, ctx=None):
    """``merge_score_protos`` (utils/protocol.py:504-525) on two device tubelet sets of one video, one launch, no host wait.

    ``a`` / ``b``: dicts with ``tracks`` [C,T,F,5] f32, ``ntracks`` [C] int32, ``anchors`` [C,T,3] f32, ``series`` (a tuple of
    1..4 f64 [C,T,F] tensors, or one tensor; series 0 is det_score) and optionally ``tboxes`` [C,T,F,4] f32 -- the keys
    ``interpolate_tracks`` returns, whose result goes in unchanged.  The sets share C, F, the number of series and the presence
    of tboxes; Ta and Tb may differ; ``a is b`` is fine; the inputs are never modified.
      'combine': a's tubelets, then b's: T_out = Ta + Tb, out slot t < nta[c] is a's slot t, slot nta[c] + u is b's slot u,
        ntracks = nta + ntb; the slots behind are NaN (zero anchors).  Copies are bit for bit.
      'max': the output has a's shape; in slot t < min(nta[c], ntb[c]) the i-th box of a meets the i-th box of b and takes all
        of b's values (row, tboxes, every series) where det_b > det_a (NaN, equal scores, -0.0 vs +0.0 keep a); everything
        else is a's.  Paired boxes must lie on the same frames and the slots' anchor frames must be equal, else ValueError
        when the call -- or with ``sync=False`` a later ``ctx.sync()`` -- waits (the slot is then a copy of a).
    Semantics in full: include/vdet_hip.h (vdet_merge_tracks).  Returns a dict of the same form (``tracks``, ``ntracks``,
    ``anchors``, ``series``, ``tboxes`` when the inputs have them), plus ``from_b`` [C,T,F] uint8 for 'max'."""
    if scheme not in _MERGE_SCHEMES:
        raise ValueError("scheme must be 'combine' or 'max'")
    sa, sb = _merge_set(a, 'a'), _merge_set(b, 'b')
    C, Ta, F = sa[0].shape[0], sa[0].shape[1], sa[0].shape[2]
    Tb = sb[0].shape[1]
    if sb[0].shape[0] != C or sb[0].shape[2] != F:
        raise ValueError("a and b must share C and F (a: C=%d F=%d, b: C=%d F=%d)" % (C, F, sb[0].shape[0], sb[0].shape[2]))
    if len(sa[4]) != len(sb[4]):
        raise ValueError("a and b must have the same number of series")
    if (sa[3] is None) != (sb[3] is None):
        raise ValueError("tboxes: in both sets or in neither")
    _same_gpu(sa[:4] + sa[4] + sb[:4] + sb[4], "every tensor of a and b")
    cont = lambda s: tuple(None if x is None else x.contiguous() for x in s[:4]) + (tuple(x.contiguous() for x in s[4]),)
    sa, sb = cont(sa), cont(sb)
    ctx = _ctx_for(sa[0], ctx)
    tracks, ntracks, anchors, tboxes, series, from_b, To = _merge_call(ctx, scheme, np.array([0, F], dtype=np.int64), C, Ta, Tb, sa,
                                                                       sb, sync)
    out = dict(tracks=tracks.view(C, To, F, 5), ntracks=ntracks.view(C), anchors=anchors.view(C, To, 3),
               series=tuple(series[q].view(C, To, F) for q in range(series.shape[0])))
    if tboxes is not None:
        out['tboxes'] = tboxes.view(C, To, F, 4)
    if from_b is not None:
        out['from_b'] = from_b.view(C, To, F)
    return out


def merge_tracks_batch(batch_a, batch_b, scheme='combine', sync=True, ctx=None):
    """``merge_tracks`` for every video of two dicts in ``video_batch``'s layout (``_batch_read``) in ONE launch.  Both dicts need
    ``tracks``, ``det`` (series 0), ``ntracks``, ``anchors`` and the same ``frame_off``; ``pooled`` (a second series) and
    ``tboxes`` are taken when BOTH have them.  Per video the bits are ``merge_tracks``' on that video alone.  Returns a dict in
    the same layout: ``tracks`` / ``det`` / ``pooled`` / ``tboxes`` (and ``from_b`` for 'max') with T_out slots, ``anchors``
    [V,C,T_out,3], ``ntracks``, ``frame_off``."""
    if scheme not in _MERGE_SCHEMES:
        raise ValueError("scheme must be 'combine' or 'max'")
    a, b = _batch_read(batch_a, 'batch_a', ('anchors', 'det')), _batch_read(batch_b, 'batch_b', ('anchors', 'det'))
    if a.o != b.o:
        raise ValueError("batch_a and batch_b must have the same frame_off")
    if a.C != b.C:
        raise ValueError("batch_a and batch_b must share C")
    off, C = a.off, a.C
    names = ['det'] + (['pooled'] if batch_a.get('pooled') and batch_b.get('pooled') else [])
    with_tb = bool(batch_a.get('tboxes')) and bool(batch_b.get('tboxes'))

    def side(bo, x, who):
        ser = tuple(_batch_field(x, bo[k], 1, _F64, k, who) for k in names)
        return x.tracks, x.ntracks, x.anchors, _batch_field(x, bo['tboxes'], 4, _F32, 'tboxes', who) if with_tb else None, ser
    sa, sb = side(batch_a, a, 'batch_a'), side(batch_b, b, 'batch_b')
    _same_gpu([x for s in (sa, sb) for x in s[:4] + s[4] if x is not None], "every tensor of batch_a and batch_b")
    ctx = _ctx_for(a.tracks, ctx)
    tracks, ntracks, anchors, tboxes, series, from_b, To = _merge_call(ctx, scheme, off, C, a.T, b.T, sa, sb, sync)
    views = lambda flat, per: _batch_views(flat, off, C, To, per)
    out = dict(tracks=views(tracks, 5), det=views(series[0], 1), pooled=views(series[1], 1) if len(names) > 1 else [],
               tboxes=views(tboxes, 4) if with_tb else [], anchors=anchors, ntracks=ntracks, frame_off=off)
    if from_b is not None:
        out['from_b'] = views(from_b, 1)
    return out


_TN_MAX = 1024         # include/vdet_hip.h: top_still + T and R per (frame, class) list; the evaluator's tracks-per-list limit


def _tn_still(still, Ft, C, T, top_still):
    """The still-image source of nms_tracks, checked: ((boxes, scores, keep_idx, keep_cnt) or None, B, keep capacity, top_still)."""
    if still is None:
        if top_still not in (None, 0):
            raise ValueError("top_still needs the still-image source (still=(boxes, scores, keep_idx, keep_cnt))")
        return None, 0, 0, 0
    if not isinstance(still, (tuple, list)) or len(still) != 4 or not all(torch.is_tensor(x) for x in still):
        raise ValueError("still must be (boxes, scores, keep_idx, keep_cnt)")
    boxes, scores, keep_idx, keep_cnt = still
    if boxes.dtype != torch.float32 or scores.dtype != torch.float32:
        raise ValueError("Buffer dtype mismatch, expected 'float32_t'")
    if boxes.dim() != 3 or tuple(boxes.shape[::2]) != (Ft, 4) or boxes.shape[1] < 1:
        raise ValueError("still: boxes must be float32 [F,B,4] over the frames of the tubelets (F = %d)" % Ft)
    B = boxes.shape[1]
    if B > 32767:
        raise ValueError("B = %d boxes per frame; the limit is 32767" % B)
    if tuple(scores.shape) != (Ft, B, C):
        raise ValueError("still: scores must be float32 [F,B,C] (layout 'FBC' only)")
    if keep_idx.dtype != torch.int32 or keep_idx.dim() != 3 or tuple(keep_idx.shape[:2]) != (Ft, C) or keep_idx.shape[2] < 1:
        raise ValueError("still: keep_idx must be int32 [F,C,cap]")
    if keep_cnt.dtype != torch.int32 or tuple(keep_cnt.shape) != (Ft, C):
        raise ValueError("still: keep_cnt must be int32 [F,C]")
    kcap = keep_idx.shape[2]
    if top_still is None:
        top_still = max(min(kcap, _TN_MAX - T), 0)
    top_still = int(top_still)
    if top_still < 0:
        raise ValueError("top_still must not be negative")
    return (boxes, scores, keep_idx, keep_cnt), B, kcap, top_still


def _tn_limits(C, T, Ft, top_still, cap):
    if top_still + T > _TN_MAX:
        raise ValueError("top_still + T = %d candidates per (frame, class); the limit is %d" % (top_still + T, _TN_MAX))
    R = max(top_still + T, 1) if cap is None else int(cap)
    if not 1 <= R <= _TN_MAX:
        raise ValueError("cap = %d output rows per (frame, class); 1 .. %d" % (R, _TN_MAX))
    if max(C * R * Ft, C * T * Ft) >= 2 ** 31 - 16:
        raise ValueError("too many tubelet boxes (C*cap*F and C*T*F must stay below 2^31 - 16)")
    return R


def _tn_tubelets(tracks, ntracks, score, tboxes, per_slot=False):
    """The tubelet source of nms_tracks / soft_nms_tracks / nms_tubelets, checked -- tensors, or a ``merge_tracks`` /
    ``interpolate_tracks`` dict as ``tracks``: (tracks, ntracks, score, tboxes, C, T, F).  ``per_slot``: a score [C,T] is as good
    as one [C,T,F]."""
    if isinstance(tracks, dict):
        d = tracks
        if ntracks is not None or any(k not in d for k in ('tracks', 'ntracks')):
            raise ValueError("a tubelet dict needs tracks and ntracks, and takes the place of both arguments")
        if not torch.is_tensor(score):
            ser = d.get('series')
            ser = (ser,) if torch.is_tensor(ser) else tuple(ser or ())
            q = 0 if score is None else score
            if not isinstance(q, int) or not 0 <= q < len(ser):
                raise ValueError("score must name one of the dict's %d series by index, or be a tensor" % len(ser))
            score = ser[q]
        tracks, ntracks, tboxes = d['tracks'], d['ntracks'], (d.get('tboxes') if tboxes is None else tboxes)
    if not torch.is_tensor(tracks) or tracks.dtype != torch.float32 or tracks.dim() != 4 or tracks.shape[3] != 5:
        raise ValueError("tracks must be float32 [C,T,F,5]")
    C, T, F = tracks.shape[0], tracks.shape[1], tracks.shape[2]
    if C < 1 or F < 1:
        raise ValueError("at least one class and one frame")
    if not torch.is_tensor(ntracks) or ntracks.dtype != torch.int32 or tuple(ntracks.shape) != (C,):
        raise ValueError("ntracks must be int32 [C]")
    shapes = ((C, T, F), (C, T)) if per_slot else ((C, T, F),)
    if not torch.is_tensor(score) or score.dtype not in (torch.float32, torch.float64) or tuple(score.shape) not in shapes:
        raise ValueError("score must be float32 / float64 [C,T,F]" + (" or [C,T]" if per_slot else ""))
    if tboxes is not None and (not torch.is_tensor(tboxes) or tboxes.dtype != torch.float32 or tuple(tboxes.shape) != (C, T, F, 4)):
        raise ValueError("tboxes must be float32 [C,T,F,4]")
    return tracks, ntracks, score, tboxes, C, T, F


_SN_METHODS = ('linear', 'gauss')       # include/vdet_hip.h: vdet_soft_nms_tracks
_SN_SIGMA_MIN = 1.0 / 64


def _sn_settings(method, thresh, sigma, min_score):
    """The scalar arguments of soft_nms_tracks, checked against the limits of include/vdet_hip.h: (method code, sigma, min_score)."""
    if method not in _SN_METHODS:
        raise ValueError("method must be 'linear' or 'gauss'")
    try:
        thresh, sigma, min_score = float(thresh), float(sigma), float(min_score)
    except (TypeError, ValueError):
        raise ValueError("thresh, sigma and min_score must be numbers")
    if not math.isfinite(sigma) or sigma < _SN_SIGMA_MIN:
        raise ValueError("sigma = %r; finite and at least 1/64" % sigma)
    if math.isnan(thresh) or math.isnan(min_score):
        raise ValueError("thresh and min_score must not be NaN")
    return _SN_METHODS.index(method), sigma, min_score


_VN_WEIGHTS = ('score', 'uniform')      # include/vdet_hip.h: vdet_vote_nms_tracks


def _vn_settings(vote_thresh, weights):
    """The scalar arguments of vote_nms_tracks, checked against the limits of include/vdet_hip.h: (vote_thresh, weights code)."""
    if weights not in _VN_WEIGHTS:
        raise ValueError("weights must be 'score' or 'uniform'")
    try:
        vote_thresh = float(vote_thresh)
    except (TypeError, ValueError):
        raise ValueError("vote_thresh must be a number")
    if math.isnan(vote_thresh):
        raise ValueError("vote_thresh must not be NaN")
    return vote_thresh, _VN_WEIGHTS.index(weights)


# The per-row outputs every rule on the per-frame lists writes: (key, elements per row, dtype), in the header's order.
_TN_ROWS = (('tracks', 5, torch.float32), ('score', 1, torch.float64), ('src', 1, torch.int32))

# A rule, described once: its C function (the batch form is NAME_batch), the check of its own arguments -- which returns the
# scalars that follow R in include/vdet_hip.h -- and its own per-row outputs, which follow the common ones there.
_TN_RULES = {
    'hard': ('vdet_nms_tracks', lambda: (), ()),
    'soft': ('vdet_soft_nms_tracks', _sn_settings, (('score0', 1, torch.float64),)),
    'vote': ('vdet_vote_nms_tracks', _vn_settings, (('box0', 4, torch.float32), ('votes', 1, torch.int32))),
}


def _tn_run(rule, own, off, C, T, tracks, ntracks, score, tboxes, still, thresh, top_still, cap, sync, ctx):
    """What the two forms share behind their tubelet source: the still-image source and the limits checked, the rule's ``own``
    arguments checked, one device, contiguous tensors, the launch.  Returns (R, ``_tn_call``'s flat outputs)."""
    Ft = int(off[-1])
    still, B, kcap, top_still = _tn_still(still, Ft, C, T, top_still)
    R = _tn_limits(C, T, Ft, top_still, cap)
    scalars = _TN_RULES[rule][1](*own)
    _same_gpu([ntracks, tracks, score, tboxes] + list(still or ()), "every tensor")
    tracks, ntracks, score = tracks.contiguous(), ntracks.contiguous(), score.contiguous()
    tboxes = None if tboxes is None else tboxes.contiguous()
    still = None if still is None else tuple(x.contiguous() for x in still)
    ctx = _ctx_for(ntracks, ctx)
    return R, _tn_call(ctx, rule, scalars, off, C, T, R, tracks, ntracks, score, tboxes, still, B, kcap, top_still, thresh, sync)


def _tn_single(rule, own, tracks, ntracks, score, tboxes, still, thresh, top_still, cap, sync, ctx):
    """The single-video form of a rule: tensors or a tubelet dict in, the result dict with [C,R,F,...] views out."""
    tracks, ntracks, score, tboxes, C, T, F = _tn_tubelets(tracks, ntracks, score, tboxes)
    R, flat = _tn_run(rule, own, np.array([0, F], dtype=np.int64), C, T, tracks, ntracks, score, tboxes, still, thresh, top_still,
                      cap, sync, ctx)
    out = {k: flat[k].view((C, R, F) + ((per,) if per > 1 else ())) for k, per, _ in _TN_ROWS + _TN_RULES[rule][2]}
    out.update(cnt=flat['cnt'], ntracks=flat['ntracks'].view(C))
    return out


def _tn_batch(rule, own, batch_out, score, still, thresh, top_still, cap, use_tboxes, sync, ctx):
    """The batch form of a rule: a dict in ``video_batch``'s layout in, one out."""
    b = _batch_read(batch_out)
    sv = batch_out.get(score) if isinstance(score, str) else None
    if not sv:
        raise ValueError("score must name a per-video series of batch_out (e.g. 'pooled', 'det')")
    sc = _batch_field(b, sv, 1, _F32_F64, score, 'batch_out')
    bv = batch_out.get('tboxes') if use_tboxes else None
    tboxes = _batch_field(b, bv, 4, _F32, 'tboxes', 'batch_out') if bv else None
    R, flat = _tn_run(rule, own, b.off, b.C, b.T, b.tracks, b.ntracks, sc, tboxes, still, thresh, top_still, cap, sync, ctx)
    out = {k: _batch_views(flat[k], b.off, b.C, R, per) for k, per, _ in _TN_ROWS + _TN_RULES[rule][2]}
    out.update(cnt=flat['cnt'], ntracks=flat['ntracks'], frame_off=b.off)
    return out


def _tn_call(ctx, rule, scalars, off, C, T, R, tracks, ntracks, score, tboxes, still, B, kcap, top_still, thresh, sync):
    """Allocate the outputs (flat, batch layout) and enqueue the one launch of ``rule``; every tensor contiguous and on one
    device.  The arguments go in the order include/vdet_hip.h declares them: the common inputs, the rule's scalars, the common
    outputs, the rule's outputs.  Returns the flat outputs by key: the per-row ones of ``_TN_ROWS`` and of the rule, ``cnt``
    [C,Ftot] and ``ntracks`` [V,C]."""
    V, Ft = len(off) - 1, int(off[-1])
    dev = ntracks.device
    name, _, own_rows = _TN_RULES[rule]
    out = {k: torch.empty((C * R * Ft * per,), dtype=dt, device=dev) for k, per, dt in _TN_ROWS + own_rows}
    out['cnt'] = torch.empty((C, Ft), dtype=torch.int32, device=dev)
    out['ntracks'] = torch.empty((V, C), dtype=torch.int32, device=dev)
    ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None
    sp = [ptr(x) for x in still] if still is not None and top_still > 0 else [None] * 4
    inputs = (C, T, ptr(tracks), ntracks.data_ptr(), ptr(score), int(score.dtype == torch.float64), ptr(tboxes), sp[0], sp[1], B,
              sp[2], sp[3], kcap, top_still if still is not None else 0, float(thresh), R)
    common = tuple(out[k].data_ptr() for k, _, _ in _TN_ROWS) + (out['cnt'].data_ptr(), out['ntracks'].data_ptr())
    args = inputs + tuple(scalars) + common + tuple(out[k].data_ptr() for k, _, _ in own_rows)
    if V == 1:
        ctx.check(getattr(ctx.lib, name)(ctx.h, Ft, *args))
    else:
        ctx.check(getattr(ctx.lib, name + '_batch')(ctx.h, off.ctypes.data, V, *args))
    if sync:
        ctx.sync()
    return out


def nms_tracks(tracks, ntracks=None, score=None, tboxes=None, still=None, thresh=0.5, top_still=None, cap=None, sync=True, ctx=None):
    """Per-frame NMS of tubelet boxes together with still-image detections (``apply_vid_nms`` / ``vid_nms``, utils/nms.pyx:71-125,
    as arrays): one list of detections per frame and class, one launch, no host wait.

    tracks [C,T,F,5] f32, ntracks [C] int32, score [C,T,F] f32 / f64 (``pooled``, ``det``, a TCN output: the series that scores
    the tubelet boxes), tboxes [C,T,F,4] f32 (the boxes to use instead of the track rows).  A ``merge_tracks`` /
    ``interpolate_tracks`` dict goes in as ``tracks`` (then ``ntracks`` stays None, ``score`` is the index of the series,
    default 0, or a tensor; the dict's tboxes are used unless ``tboxes`` is given).  ``still`` = (boxes [F,B,4] f32, scores
    [F,B,C] f32, keep_idx [F,C,k] int32, keep_cnt [F,C] int32): NMS survivors as ``DetEvaluator.add_keep_lists`` takes them
    ('FBC'); the first ``top_still`` of every list take part (default min(k, 1024 - T)).  T = 0 is the still-image source alone.
    The rows of a list are the still-image rows, then the tubelet rows by slot; a NaN score is no row.  Result: nms of the
    reference (f32, +1 areas, suppression iff ovr >= thresh, descending score, ties by descending row) -- semantics in full:
    include/vdet_hip.h (vdet_nms_tracks).  ``cap``: output rows per list (default top_still + T, which cannot overflow; fewer
    than a list keeps raises ValueError at the wait).  An evaluated zero-union pair raises ZeroDivisionError, a keep count or
    index out of range ValueError, when the call -- or with ``sync=False`` a later ``ctx.sync()`` -- waits.

    Returns a dict in the tubelet layout with the RANK as the slot axis: ``tracks`` [C,R,F,5] f32 (x1,y1,x2,y2,f32 score),
    ``score`` [C,R,F] f64 (the source's own score), ``src`` [C,R,F] int32 (b >= 0: still-image box b; -(t+1): tubelet slot t;
    INT32_MIN behind the count), ``cnt`` [C,F] int32, ``ntracks`` [C] int32 -- NaN behind the counts.  ``tracks`` / ``ntracks`` /
    ``score`` feed every consumer of tubelets; ``DetEvaluator.add_detections`` takes the dict."""
    return _tn_single('hard', (), tracks, ntracks, score, tboxes, still, thresh, top_still, cap, sync, ctx)


def nms_tracks_batch(batch_out, score='pooled', still=None, thresh=0.5, top_still=None, cap=None, use_tboxes=True, sync=True,
                     ctx=None):
    """``nms_tracks`` for every video of a dict in ``video_batch``'s layout (``_batch_read``) in ONE launch.  ``score`` names the
    field of the dict that scores the tubelet boxes ('pooled', 'det', ...: f32 or f64); the dict's ``tboxes`` are the boxes when
    it has them and ``use_tboxes`` holds.  ``still`` as in ``nms_tracks``, frame-major over all videos ([Ftot,...]: what
    ``video_batch`` takes and returns).  Per video the bits are ``nms_tracks``' on that video alone.  Returns ``tracks`` /
    ``score`` / ``src`` in the same layout with the rank as the slot axis ([C,R,F_v,...]), ``cnt`` [C,Ftot], ``ntracks`` [V,C]
    and ``frame_off``."""
    return _tn_batch('hard', (), batch_out, score, still, thresh, top_still, cap, use_tboxes, sync, ctx)


_TUBE_NORMS = {'union': 0, 'shared': 1, 'min': 2}       # include/vdet_hip.h: VDET_TUBE_NORM_*
_TUBE_REDUCES = {'mean': 1, 'max': 2}                   # VDET_TUBE_SCORE_MEAN / _MAX (0, VDET_TUBE_SCORE_SLOT: a score per slot)
_TUBE_MAX_T = 256


def _tube_settings(thresh, norm, reduce, min_shared, C, T, Ft, V=1):
    """The scalar arguments and the shape of nms_tubelets, checked against the limits of include/vdet_hip.h: (thresh, norm code,
    reduce code, min_shared)."""
    if norm not in _TUBE_NORMS:
        raise ValueError("norm must be 'union', 'shared' or 'min'")
    if reduce not in _TUBE_REDUCES:
        raise ValueError("reduce must be 'mean' or 'max'")
    try:
        thresh = float(thresh)
    except (TypeError, ValueError):
        raise ValueError("thresh must be a number")
    if thresh != thresh:
        raise ValueError("thresh must not be NaN")
    if isinstance(min_shared, bool) or not isinstance(min_shared, (int, np.integer)) or min_shared < 1:
        raise ValueError("min_shared must be an integer >= 1")
    if not 1 <= T <= _TUBE_MAX_T:
        raise ValueError("T = %d tubelet slots per class; 1 .. %d" % (T, _TUBE_MAX_T))
    if V > 65535:
        raise ValueError("at most 65535 videos in one call")
    if max(C * T * Ft, V * C * T) >= 2 ** 31 - 16:
        raise ValueError("too many tubelet boxes (C*T*F must stay below 2^31 - 16)")
    return thresh, _TUBE_NORMS[norm], _TUBE_REDUCES[reduce], int(min_shared)


def _tube_call(ctx, off, C, T, tracks, ntracks, tboxes, score, mode, anchors, series, thresh, norm, min_shared, return_overlaps,
               sync):
    """Allocate the outputs (flat, batch layout) and enqueue the launches; every tensor contiguous and on one device.  Returns
    (tracks, ntracks [V,C], tboxes or None, anchors [V,C,T,3] or None, series [n, N], src, tscore, by [V,C,T], overlaps
    [V,C,T,T] or None)."""
    V, Ft = len(off) - 1, int(off[-1])
    dev = tracks.device
    n, N = len(series), C * T * Ft
    otracks = torch.empty((N * 5,), dtype=torch.float32, device=dev)
    ont = torch.empty((V, C), dtype=torch.int32, device=dev)
    otboxes = torch.empty((N * 4,), dtype=torch.float32, device=dev) if tboxes is not None else None
    oanchors = torch.empty((V, C, T, 3), dtype=torch.float32, device=dev) if anchors is not None else None
    oseries = torch.empty((n, N), dtype=torch.float64, device=dev)
    src = torch.empty((V, C, T), dtype=torch.int32, device=dev)
    tscore = torch.empty((V, C, T), dtype=torch.float64, device=dev)
    by = torch.empty((V, C, T), dtype=torch.int32, device=dev)
    ov = torch.empty((V, C, T, T), dtype=torch.float64, device=dev) if return_overlaps else None
    ps = (ctypes.c_void_p * 4)(*[x.data_ptr() for x in series])
    ptr = lambda x: x.data_ptr() if x is not None else None
    tail = (C, T, tracks.data_ptr(), ntracks.data_ptr(), ptr(tboxes), score.data_ptr(), int(score.dtype == torch.float64), mode,
            ptr(anchors), ps, n, thresh, norm, min_shared, otracks.data_ptr(), ont.data_ptr(), ptr(otboxes), ptr(oanchors),
            oseries.data_ptr() if n else None, src.data_ptr(), tscore.data_ptr(), by.data_ptr(), ptr(ov))
    if V == 1:
        ctx.check(ctx.lib.vdet_nms_tubelets(ctx.h, Ft, *tail))
    else:
        ctx.check(ctx.lib.vdet_nms_tubelets_batch(ctx.h, off.ctypes.data, V, *tail))
    if sync:
        ctx.sync()
    return otracks, ont, otboxes, oanchors, oseries, src, tscore, by, ov


def nms_tubelets(tracks, ntracks=None, score=None, tboxes=None, anchors=None, series=None, thresh=0.5, norm='union', reduce='mean',
                 min_shared=1, return_overlaps=False, sync=True, ctx=None):
    """NMS over WHOLE tubelets by spatio-temporal overlap: per class, a tubelet that repeats a better-scored one is dropped, the
    survivors are compacted into score order.  The stage behind ``track_from_anchors`` / ``track_pixels`` / ``merge_tracks`` and
    in front of the scorers; no host wait.  The rule is the project's own -- in full: include/vdet_hip.h (vdet_nms_tubelets),
    in numpy: tests/tubenms_spec.py.

    tracks [C,T,F,5] f32, ntracks [C] int32, tboxes [C,T,F,4] f32 (the boxes to use instead of the track rows), anchors [C,T,3]
    f32 and ``series`` (up to 4 f64 [C,T,F] tensors, or one tensor) travel with the kept tubelets.  ``score`` (f32 / f64): [C,T]
    -- a score per tubelet -- or [C,T,F], reduced by ``reduce`` ('mean' / 'max') over the frames where the box exists and the
    value is not NaN.  A ``merge_tracks`` / ``interpolate_tracks`` dict goes in as ``tracks`` (then ``ntracks`` stays None,
    ``score`` is the index of a series, default 0, or a tensor; the dict's tboxes, anchors and series are used unless given).
    A tubelet without a box or with a NaN score is absent: neither kept nor suppressing.
      overlap of two tubelets = (sum over the shared frames of the f32 IoU, in units of 2^-24) / den, with den by ``norm``:
        'union'  frames on which either has a box (the usual spatio-temporal IoU),
        'shared' frames on which both have one,
        'min'    the boxes of the shorter (a short tubelet inside a long one overlaps fully);
      0 with fewer than ``min_shared`` shared frames.  Greedy in descending score (ties by descending slot): suppression iff
      overlap >= thresh; thresh > 1 only sorts.

    Returns a dict of ``merge_tracks``' form -- ``tracks``, ``ntracks``, and ``tboxes`` / ``anchors`` / ``series`` when given:
    slot r is a bit-for-bit copy of source slot ``src[c,r]``, NaN rows (zero anchors) behind the count -- plus ``src`` [C,T]
    int32 (INT32_MIN behind the count), ``tscore`` [C,T] f64, ``by`` [C,T] int32 by INPUT slot (itself if kept, the slot that
    suppressed it, -1 if absent) and, with ``return_overlaps``, ``overlaps`` [C,T,T] f64 (NaN rows and columns for absent
    slots).  The result feeds ``merge_tracks``, ``nms_tracks``, ``rescore_tubelets``, ``tcn_tracks``, ``DetEvaluator.add_tracks``."""
    if isinstance(tracks, dict):
        anchors = tracks.get('anchors') if anchors is None else anchors
        series = tracks.get('series') if series is None else series
    tracks, ntracks, score, tboxes, C, T, F = _tn_tubelets(tracks, ntracks, score, tboxes, per_slot=True)
    if anchors is not None and (not torch.is_tensor(anchors) or anchors.dtype != torch.float32 or tuple(anchors.shape) != (C, T, 3)):
        raise ValueError("anchors must be float32 [C,T,3]")
    if series is None or (isinstance(series, (tuple, list)) and not series):
        series = ()
    else:
        series = _merge_series(series, (C, T, F), 'nms_tubelets')
    thresh, norm, mode, min_shared = _tube_settings(thresh, norm, reduce, min_shared, C, T, F)
    _same_gpu((tracks, ntracks, score, tboxes, anchors) + series, "every tensor")
    cont = lambda x: None if x is None else x.contiguous()
    tracks, ntracks, score, tboxes, anchors = cont(tracks), cont(ntracks), cont(score), cont(tboxes), cont(anchors)
    series = tuple(x.contiguous() for x in series)
    ctx = _ctx_for(tracks, ctx)
    ot, ont, otb, oan, oser, src, tscore, by, ov = _tube_call(
        ctx, np.array([0, F], dtype=np.int64), C, T, tracks, ntracks, tboxes, score, mode if score.dim() == 3 else 0, anchors, series,
        thresh, norm, min_shared, return_overlaps, sync)
    out = dict(tracks=ot.view(C, T, F, 5), ntracks=ont.view(C), src=src.view(C, T), tscore=tscore.view(C, T), by=by.view(C, T))
    if otb is not None:
        out['tboxes'] = otb.view(C, T, F, 4)
    if oan is not None:
        out['anchors'] = oan.view(C, T, 3)
    if series:
        out['series'] = tuple(oser[q].view(C, T, F) for q in range(len(series)))
    if ov is not None:
        out['overlaps'] = ov.view(C, T, T)
    return out


def nms_tubelets_batch(batch_out, score='det', thresh=0.5, norm='union', reduce='mean', min_shared=1, return_overlaps=False,
                       sync=True, ctx=None):
    """``nms_tubelets`` for every video of a dict in ``video_batch``'s layout (``_batch_read``) in ONE call.  ``score`` names the
    field of the dict that scores the tubelets ('det', 'pooled', ...: per-video [C,T,F_v] views, f32 or f64, reduced by
    ``reduce``), or is a tensor [V,C,T] with a score per tubelet.  The dict's ``tboxes`` are the boxes when it has them;
    ``det`` / ``pooled`` (f64), ``tboxes`` and ``anchors`` travel with the kept tubelets when present.  Per
    video the bits are ``nms_tubelets``' on that video alone.  Returns the same layout -- ``tracks``, ``det``, ``pooled``,
    ``tboxes`` (empty lists for what the input lacks), ``anchors`` (None without), ``ntracks`` [V,C], ``frame_off`` -- plus
    ``src`` / ``tscore`` / ``by`` [V,C,T] and, with ``return_overlaps``, ``overlaps`` [V,C,T,T]."""
    with_anchors = isinstance(batch_out, dict) and batch_out.get('anchors') is not None
    b = _batch_read(batch_out, need=('anchors',) if with_anchors else ())
    off, V, Ft, C, T, tracks, ntracks, anchors = b.off, b.V, b.Ft, b.C, b.T, b.tracks, b.ntracks, b.anchors
    if isinstance(score, str):
        sv = batch_out.get(score)
        if not sv:
            raise ValueError("score must name a per-video series of batch_out (e.g. 'det', 'pooled') or be a tensor [V,C,T]")
        sc, per_frame = _batch_field(b, sv, 1, _F32_F64, score, 'batch_out'), True
    else:
        if not torch.is_tensor(score) or score.dtype not in _F32_F64 or tuple(score.shape) != (V, C, T):
            raise ValueError("score must name a per-video series of batch_out (e.g. 'det', 'pooled') or be a tensor [V,C,T]")
        sc, per_frame = score.contiguous(), False
    names = [k for k in ('det', 'pooled') if batch_out.get(k)]
    series = tuple(_batch_field(b, batch_out[k], 1, _F64, k, 'batch_out') for k in names)
    bv = batch_out.get('tboxes')
    tboxes = _batch_field(b, bv, 4, _F32, 'tboxes', 'batch_out') if bv else None
    thresh, norm, mode, min_shared = _tube_settings(thresh, norm, reduce, min_shared, C, T, Ft, V)
    _same_gpu((tracks, ntracks, sc, tboxes, anchors) + series, "every tensor")
    ctx = _ctx_for(tracks, ctx)
    ot, ont, otb, oan, oser, src, tscore, by, ov = _tube_call(
        ctx, off, C, T, tracks, ntracks, tboxes, sc, mode if per_frame else 0, anchors, series, thresh, norm, min_shared,
        return_overlaps, sync)
    views = lambda flat, per: _batch_views(flat, off, C, T, per)
    ser = {k: views(oser[q], 1) for q, k in enumerate(names)}
    out = dict(tracks=views(ot, 5), det=ser.get('det', []), pooled=ser.get('pooled', []), tboxes=views(otb, 4) if otb is not None else [],
               anchors=oan, ntracks=ont, frame_off=off, src=src, tscore=tscore, by=by)
    if ov is not None:
        out['overlaps'] = ov
    return out


def soft_nms_tracks(tracks, ntracks=None, score=None, tboxes=None, still=None, method='linear', thresh=0.3, sigma=0.5,
                    min_score=0.001, top_still=None, cap=None, sync=True, ctx=None):
    """Soft-NMS (Bodla et al., ICCV 2017) of the per-frame detection lists ``nms_tracks`` builds: a row that overlaps a better
    one keeps its place in the list with a DECAYED score instead of being deleted.  One launch, no host wait.  The reference
    library has no function for it; the rule in full: include/vdet_hip.h (vdet_soft_nms_tracks); tests/softnms_spec.py states it
    in numpy float32 and the device matches it on bits.

    Every argument up to ``still``, ``top_still`` and ``cap`` as in ``nms_tracks`` (a ``merge_tracks`` / ``interpolate_tracks``
    dict goes in as ``tracks``); the rows of a list and their order are its rows.  Rows below ``min_score`` are removed; then,
    round after round, the alive row with the largest current f32 score (ties by descending row) is emitted and every other
    alive row j is decayed by its overlap ovr with it: ``'linear'`` s_j *= 1 - ovr iff ovr >= ``thresh`` (the project's ``>=``;
    the paper's code tests ``>``), ``'gauss'`` s_j *= exp(-ovr^2 / ``sigma``) for every pair (``thresh`` unused; ``sigma`` >=
    1/64).  A score that falls below ``min_score`` (or becomes NaN) removes the row; ``min_score=-inf`` keeps every row.  The
    rule is multiplicative and meant for scores >= 0: a negative score RISES towards zero when decayed -- map margins into
    [0, 1] first where that matters.

    The defaults -- ``method='linear'``, ``thresh=0.3``, ``sigma=0.5``, ``min_score=0.001`` -- are recalled from the paper's
    public code and could not be checked here.

    Returns a dict in ``nms_tracks``' rank layout: ``tracks`` [C,R,F,5] f32 (box, decayed f32 score), ``score`` [C,R,F] f64 (the
    decayed score widened), ``score0`` [C,R,F] f64 (the source's own unrounded score: what ``nms_tracks`` calls ``score``),
    ``src`` [C,R,F] int32, ``cnt`` [C,F] int32 (rows emitted), ``ntracks`` [C] int32 -- NaN / INT32_MIN behind the counts.
    ``DetEvaluator.add_detections`` takes the dict; ``seq_nms`` / ``top_anchors`` / ``nms_tracks`` take its tracks / ntracks /
    score.  ``cap`` below a list's count raises ValueError at the wait (the counts are written), an evaluated zero-union pair
    ZeroDivisionError, a keep count or index out of range ValueError."""
    return _tn_single('soft', (method, thresh, sigma, min_score), tracks, ntracks, score, tboxes, still, thresh, top_still, cap,
                      sync, ctx)


def soft_nms_tracks_batch(batch_out, score='pooled', still=None, method='linear', thresh=0.3, sigma=0.5, min_score=0.001,
                          top_still=None, cap=None, use_tboxes=True, sync=True, ctx=None):
    """``soft_nms_tracks`` for every video of a dict in ``video_batch``'s layout (``_batch_read``) in ONE launch; the inputs as in
    ``nms_tracks_batch``.  Per video the bits are ``soft_nms_tracks``' on that video alone.  Returns ``tracks`` / ``score`` /
    ``score0`` / ``src`` in the same layout with the rank as the slot axis ([C,R,F_v,...]), ``cnt`` [C,Ftot], ``ntracks`` [V,C]
    and ``frame_off``."""
    return _tn_batch('soft', (method, thresh, sigma, min_score), batch_out, score, still, thresh, top_still, cap, use_tboxes,
                     sync, ctx)


def vote_nms_tracks(tracks, ntracks=None, score=None, tboxes=None, still=None, thresh=0.5, top_still=None, cap=None,
                    vote_thresh=0.5, weights='score', sync=True, ctx=None):
    """Bounding-box voting (Gidaris & Komodakis, ICCV 2015) on the per-frame detection lists ``nms_tracks`` builds: the hard NMS
    at ``thresh`` decides which rows are kept, their order and their scores -- exactly ``nms_tracks``' -- and every kept row's
    BOX becomes the weighted mean of the boxes of the list's rows that overlap it, the suppressed ones included.  One launch,
    no host wait.  The reference library has no function for it; the rule in full: include/vdet_hip.h (vdet_vote_nms_tracks);
    tests/votenms_spec.py states it in numpy and the device matches it on bits.

    Every argument up to ``cap`` as in ``nms_tracks`` (a ``merge_tracks`` / ``interpolate_tracks`` dict goes in as ``tracks``).
    The voters of a kept row are the row itself and every other present row whose overlap with it (the reference's f32 ovr,
    the kept row as box i) is >= ``vote_thresh``; a zero union or a NaN overlap is no voter and raises nothing.  ``weights``:
    ``'score'`` weighs a voter by its f32 score where that is > 0 and by nothing otherwise, ``'uniform'`` by 1.  The sums run
    in float64 over the voters in ascending row index; a row whose weights sum to 0, or whose mean is not finite, keeps its own
    box.  A score <= 0 therefore moves nothing under ``'score'`` -- map margins into [0, 1] first where that matters.
    ``vote_thresh`` above 1 leaves every box as it is: the result then equals ``nms_tracks``' on bits.

    Returns ``nms_tracks``' dict -- ``tracks`` [C,R,F,5] f32 now with the VOTED box beside the row's own f32 score, ``score``,
    ``src``, ``cnt``, ``ntracks`` unchanged -- plus ``box0`` [C,R,F,4] f32 (the row's own box, NaN behind the count) and
    ``votes`` [C,R,F] int32 (voters, the row itself included; 0 behind the count).  ``DetEvaluator.add_detections`` takes the
    dict; ``seq_nms`` / ``soft_nms_tracks`` / ``top_anchors`` / ``nms_tracks`` take its tracks / ntracks / score.  The errors at
    the wait are ``nms_tracks``': ``cap`` below a list's count, a zero-union pair the NMS evaluates, bad keep data."""
    return _tn_single('vote', (vote_thresh, weights), tracks, ntracks, score, tboxes, still, thresh, top_still, cap, sync, ctx)


def vote_nms_tracks_batch(batch_out, score='pooled', still=None, thresh=0.5, top_still=None, cap=None, vote_thresh=0.5,
                          weights='score', use_tboxes=True, sync=True, ctx=None):
    """``vote_nms_tracks`` for every video of a dict in ``video_batch``'s layout (``_batch_read``) in ONE launch; the inputs as in
    ``nms_tracks_batch``.  Per video the bits are ``vote_nms_tracks``' on that video alone.  Returns ``tracks`` / ``score`` /
    ``src`` / ``box0`` / ``votes`` in the same layout with the rank as the slot axis ([C,R,F_v,...]), ``cnt`` [C,Ftot],
    ``ntracks`` [V,C] and ``frame_off``: a dict in ``video_batch``'s layout again, which ``DetEvaluator.add_detections``,
    ``seq_nms_batch``, ``soft_nms_tracks_batch`` (``score='score'``), ``nms_tracks_batch`` and ``top_anchors`` take as it is."""
    return _tn_batch('vote', (vote_thresh, weights), batch_out, score, still, thresh, top_still, cap, use_tboxes, sync, ctx)


_SQ_MAX_R, _SQ_MAX_SEQS = 256, 4096     # include/vdet_hip.h: vdet_seq_nms
_SQ_RESCORE = ('avg', 'max')


def _sq_settings(C, R, Ft, V, link_thres, nms_thres, rescore, max_seqs, min_score):
    """The scalar arguments of seq_nms, checked against the limits of include/vdet_hip.h: (link, nms, rescore code, S, floor)."""
    link_thres, nms_thres, min_score = float(link_thres), float(nms_thres), float(min_score)
    if not (math.isfinite(link_thres) and math.isfinite(nms_thres)):
        raise ValueError("link_thres and nms_thres must be finite")
    if math.isnan(min_score):
        raise ValueError("min_score must not be NaN")
    if rescore not in _SQ_RESCORE:
        raise ValueError("rescore must be 'avg' or 'max'")
    S = int(max_seqs)
    if not 1 <= S <= _SQ_MAX_SEQS:
        raise ValueError("max_seqs = %d sequences per class; 1 .. %d" % (S, _SQ_MAX_SEQS))
    if C < 1 or Ft < 1:
        raise ValueError("at least one class and one frame")
    if not 1 <= R <= _SQ_MAX_R:
        raise ValueError("R = %d rows per (frame, class); 1 .. %d (cut wider lists with nms_tracks(cap=))" % (R, _SQ_MAX_R))
    if max(C * R * Ft * ((R + 31) // 32), C * S * V) >= 2 ** 31 - 16:
        raise ValueError("too many boxes (C*R*F, the link words C*F*R*ceil(R/32) and C*max_seqs*V must stay below 2^31 - 16)")
    return link_thres, nms_thres, _SQ_RESCORE.index(rescore), S, min_score


def _sq_call(ctx, off, C, R, tracks, ntracks, score, link_thres, nms_thres, rescore, S, min_score, sync):
    """Allocate the outputs (flat, batch layout) and enqueue the launches; every tensor contiguous and on one device."""
    V, Ft = len(off) - 1, int(off[-1])
    dev = ntracks.device
    N = C * R * Ft
    new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
    o = dict(tracks=new((N * 5,), torch.float32), score=new((N,), torch.float64), seq=new((N,), torch.int32),
             ntracks=new((V, C), torch.int32), nseq=new((V, C), torch.int32), seq_sum=new((V, C, S), torch.float64),
             seq_len=new((V, C, S), torch.int32), seq_end=new((V, C, S, 2), torch.int32), exhausted=new((V, C), torch.uint8))
    tail = (C, R, tracks.data_ptr(), ntracks.data_ptr(), None if score is None else score.data_ptr(),
            int(score is not None and score.dtype == torch.float64), link_thres, nms_thres, rescore, S, min_score) + \
        tuple(o[k].data_ptr() for k in ('tracks', 'score', 'seq', 'ntracks', 'nseq', 'seq_sum', 'seq_len', 'seq_end', 'exhausted'))
    if V == 1:
        ctx.check(ctx.lib.vdet_seq_nms(ctx.h, Ft, *tail))
    else:
        ctx.check(ctx.lib.vdet_seq_nms_batch(ctx.h, off.ctypes.data, V, *tail))
    if sync:
        ctx.sync()
    return o


def seq_nms(dets, ntracks=None, score=None, link_thres=0.5, nms_thres=0.3, rescore='avg', max_seqs=32, min_score=-math.inf,
            sync=True, ctx=None):
    """Seq-NMS (Han et al. 2016) of per-frame detections in the tubelet layout, per class: link the boxes of neighbouring frames
    whose IoU is >= ``link_thres``, take the sequence with the largest score sum (dynamic programming over the frames), give
    each of its boxes the sequence's average (``rescore='avg'``) or maximum (``'max'``) score, suppress the boxes of the same
    frames that overlap them by >= ``nms_thres``, and repeat on what is left -- at most ``max_seqs`` times, and only while the
    best sum is >= ``min_score``.  The rule in full: include/vdet_hip.h (vdet_seq_nms); tests/seqnms_spec.py states it in numpy
    and the device matches it on bits.  The reference library has no function for it.

    ``dets``: the dict ``nms_tracks`` returned, or any tubelet dict with ``tracks`` / ``ntracks`` (``ntracks`` stays None), or
    tracks [C,R,F,5] f32 with ntracks [C] int32.  ``score``: [C,R,F] f32 / f64, or -- with a dict -- the name of one of its
    fields or the index of one of its ``series``; default: column 4 of the boxes.  A row is a node when its slot is below
    ntracks, its x1 is not NaN and its score is finite.  R <= 256 (cut wider lists with ``nms_tracks(cap=)``), max_seqs <= 4096.

    ``link_thres`` 0.5 and ``nms_thres`` 0.3 are the paper's; ``max_seqs`` = 32 is an untuned starting point, not taken from
    anywhere.

    Returns a dict; slots stay where they were (no compaction, no re-ranking), S = max_seqs:
      tracks [C,R,F,5] f32   members of a sequence and leftovers: the input box and (float) new score; every other row NaN
      score [C,R,F] f64      the new score (a leftover keeps its own), NaN elsewhere
      seq [C,R,F] int32      k >= 0 member of sequence k, -1 leftover, -2 suppressed, INT32_MIN no node
      ntracks [C] int32      the input clamped to 0..R;   nseq [C] int32 sequences taken
      seq_sum [C,S] f64, seq_len [C,S] int32, seq_end [C,S,2] int32 (frame, slot): NaN, 0, -1 behind nseq
      exhausted [C] uint8    1 iff no node was left when the rounds ended
    ``DetEvaluator.add_detections`` takes the dict; ``top_anchors`` / ``nms_tracks`` take its tracks / ntracks / score.  No
    host wait with ``sync=False``.  ValueError before any launch for a wrong dtype, device or shape and beyond the limits."""
    tracks = dets
    if isinstance(dets, dict):
        d = dets
        if ntracks is not None or any(k not in d for k in ('tracks', 'ntracks')):
            raise ValueError("a tubelet dict needs tracks and ntracks, and takes the place of both arguments")
        if isinstance(score, str):
            if not torch.is_tensor(d.get(score)):
                raise ValueError("score must name a tensor field of the dict, one of its series by index, or be a tensor")
            score = d[score]
        elif score is not None and not torch.is_tensor(score):
            ser = d.get('series')
            ser = (ser,) if torch.is_tensor(ser) else tuple(ser or ())
            if not isinstance(score, int) or not 0 <= score < len(ser):
                raise ValueError("score must name a tensor field of the dict, one of its %d series by index, or be a tensor" % len(ser))
            score = ser[score]
        tracks, ntracks = d['tracks'], d['ntracks']
    if not torch.is_tensor(tracks) or tracks.dtype != torch.float32 or tracks.dim() != 4 or tracks.shape[3] != 5:
        raise ValueError("tracks must be float32 [C,R,F,5]")
    C, R, F = tracks.shape[0], tracks.shape[1], tracks.shape[2]
    if not torch.is_tensor(ntracks) or ntracks.dtype != torch.int32 or tuple(ntracks.shape) != (C,):
        raise ValueError("ntracks must be int32 [C]")
    if score is not None and (not torch.is_tensor(score) or score.dtype not in _F32_F64 or tuple(score.shape) != (C, R, F)):
        raise ValueError("score must be float32 / float64 [C,R,F], or None for column 4 of the boxes")
    st = _sq_settings(C, R, F, 1, link_thres, nms_thres, rescore, max_seqs, min_score)
    _same_gpu([ntracks, tracks, score], "every tensor")
    tracks, ntracks, score = tracks.contiguous(), ntracks.contiguous(), None if score is None else score.contiguous()
    ctx = _ctx_for(ntracks, ctx)
    o = _sq_call(ctx, np.array([0, F], dtype=np.int64), C, R, tracks, ntracks, score, *st, sync=sync)
    S = st[3]
    return dict(tracks=o['tracks'].view(C, R, F, 5), score=o['score'].view(C, R, F), seq=o['seq'].view(C, R, F),
                ntracks=o['ntracks'].view(C), nseq=o['nseq'].view(C), seq_sum=o['seq_sum'].view(C, S), seq_len=o['seq_len'].view(C, S),
                seq_end=o['seq_end'].view(C, S, 2), exhausted=o['exhausted'].view(C))


def seq_nms_batch(batch_dets, score=None, link_thres=0.5, nms_thres=0.3, rescore='avg', max_seqs=32, min_score=-math.inf, sync=True,
                  ctx=None):
    """``seq_nms`` for every video of a dict in ``video_batch``'s layout (``_batch_read``; what ``nms_tracks_batch`` returns) in
    the same launches.  ``score`` names the per-video field of the dict that scores the boxes ('score', 'pooled', ...: f32 or
    f64); None: column 4.  Per video the bits are ``seq_nms``' on that video alone -- no sequence crosses a video border.
    Returns ``tracks`` / ``score`` / ``seq`` as per-video views in the same layout, ``ntracks`` / ``nseq`` / ``exhausted`` [V,C],
    ``seq_sum`` / ``seq_len`` [V,C,S], ``seq_end`` [V,C,S,2] (frames counted within the video) and ``frame_off``.  The defaults
    are ``seq_nms``' (the paper's thresholds, an untuned ``max_seqs``)."""
    b = _batch_read(batch_dets, 'batch_dets')
    off, V, Ft, C, R, tracks, ntracks = b.off, b.V, b.Ft, b.C, b.T, b.tracks, b.ntracks
    sc = None
    if score is not None:
        sv = batch_dets.get(score) if isinstance(score, str) else None
        if not isinstance(sv, (list, tuple)) or not sv:
            raise ValueError("score must name a per-video series of batch_dets (e.g. 'score', 'pooled'), or be None for column 4")
        sc = _batch_field(b, sv, 1, _F32_F64, score, 'batch_dets')
    st = _sq_settings(C, R, Ft, V, link_thres, nms_thres, rescore, max_seqs, min_score)
    _same_gpu([ntracks, tracks, sc], "every tensor")
    ctx = _ctx_for(ntracks, ctx)
    o = _sq_call(ctx, off, C, R, tracks, ntracks, sc, *st, sync=sync)
    views = lambda flat, per: _batch_views(flat, off, C, R, per)
    return dict(tracks=views(o['tracks'], 5), score=views(o['score'], 1), seq=views(o['seq'], 1), ntracks=o['ntracks'],
                nseq=o['nseq'], seq_sum=o['seq_sum'], seq_len=o['seq_len'], seq_end=o['seq_end'], exhausted=o['exhausted'],
                frame_off=off)


_MOTION_BLOCKS = (8, 16, 32)       # include/vdet_hip.h: vdet_motion_field
_MOTION_MAX_REACH = 16


def motion_field(images, block=16, radius=8, sync=True, ctx=None):
    """The block-motion field of a video, both directions, with its summed table: what ``propagate_detections`` moves boxes
    along (include/vdet_hip.h: vdet_motion_field; the rule is tests/motion_spec.py).  Build it once per video.

    images uint8 [F,H,W,3], contiguous; ``block`` P in (8, 16, 32); ``radius`` R in 1 .. 16.  With Hb = ceil(H/P), Wb = ceil(W/P):
    ``field`` int16 [2,F,Hb,Wb,2] is (dx, dy) of every block's best match on the next (direction 0) and on the previous
    (direction 1) frame -- SAD of the tracker's luma over [-R,R]^2 with the image's edges replicated, the tracker's tie order (zero
    motion on flat content) --, ``cost`` int32 [2,F,Hb,Wb] its SAD, ``fsum`` int32 [2,F,Hb+1,Wb+1,2] the summed table of the field
    (row 0 and column 0 zero).  The frame without a partner is zero.  Exact.  Two launches, no host wait.

    Returns dict(field, cost, fsum, block, size=(H, W)).  ValueError for another layout, block or radius, or a video whose table
    would pass 2^31 - 16 elements (before any launch)."""
    F, H, W = _images(images)
    block, radius = int(block), int(radius)
    if block not in _MOTION_BLOCKS:
        raise ValueError("block = %d; 8, 16 or 32" % block)
    if not 1 <= radius <= 16:
        raise ValueError("radius = %d; 1 .. 16" % radius)
    Hb, Wb = -(-H // block), -(-W // block)
    if 4 * F * (Hb + 1) * (Wb + 1) >= 2 ** 31 - 16:
        raise ValueError("motion field too large (2*F*(Hb+1)*(Wb+1)*2 must stay below 2^31 - 16)")
    ctx = _ctx_for(images, ctx)
    dev = images.device
    field = torch.empty((2, F, Hb, Wb, 2), dtype=torch.int16, device=dev)
    cost = torch.empty((2, F, Hb, Wb), dtype=torch.int32, device=dev)
    fsum = torch.empty((2, F, Hb + 1, Wb + 1, 2), dtype=torch.int32, device=dev)
    ctx.check(ctx.lib.vdet_motion_field(ctx.h, images.data_ptr(), F, H, W, block, radius, field.data_ptr(), cost.data_ptr(),
                                        fsum.data_ptr()))
    if sync:
        ctx.sync()
    return dict(field=field, cost=cost, fsum=fsum, block=block, size=(H, W))


def _pd_motion(motion):
    """The checked ``motion_field`` dict of propagate_detections: (fsum, block, H, W, F, Hb, Wb).  Layout checks only."""
    if not isinstance(motion, dict) or any(k not in motion for k in ('fsum', 'block', 'size')):
        raise ValueError("motion must be the dict ops.motion_field returns (fsum, block, size)")
    fsum, block, size = motion['fsum'], motion['block'], motion['size']
    if block not in _MOTION_BLOCKS:
        raise ValueError("motion: block = %r; 8, 16 or 32" % (block,))
    if not isinstance(size, (tuple, list)) or len(size) != 2 or not all(isinstance(v, int) and 1 <= v <= 32767 for v in size):
        raise ValueError("motion: size must be (H, W) with 1 .. 32767 rows and columns")
    H, W = size
    Hb, Wb = -(-H // block), -(-W // block)
    if not torch.is_tensor(fsum) or fsum.dtype != torch.int32 or fsum.dim() != 5 or fsum.shape[1] < 1 or \
            tuple(fsum.shape) != (2, fsum.shape[1], Hb + 1, Wb + 1, 2) or not fsum.is_contiguous():
        raise ValueError("motion: fsum must be int32 [2,F,%d,%d,2], contiguous (%d x %d images in blocks of %d)" % (
            Hb + 1, Wb + 1, H, W, block))
    return fsum, block, H, W, fsum.shape[1], Hb, Wb


def _pd_still(still, Ft):
    """The still-image source of propagate_detections, checked as ``_tn_still`` checks nms_tracks': ((boxes, scores, keep_idx,
    keep_cnt), B, C, keep capacity)."""
    if not isinstance(still, (tuple, list)) or len(still) != 4 or not all(torch.is_tensor(x) for x in still):
        raise ValueError("still must be (boxes, scores, keep_idx, keep_cnt)")
    boxes, scores, keep_idx, keep_cnt = still
    if boxes.dtype != torch.float32 or scores.dtype != torch.float32:
        raise ValueError("Buffer dtype mismatch, expected 'float32_t'")
    if boxes.dim() != 3 or tuple(boxes.shape[::2]) != (Ft, 4) or boxes.shape[1] < 1:
        raise ValueError("still: boxes must be float32 [F,B,4] over the frames of the motion field (F = %d)" % Ft)
    B = boxes.shape[1]
    if B > 32767:
        raise ValueError("B = %d boxes per frame; the limit is 32767" % B)
    if scores.dim() != 3 or tuple(scores.shape[:2]) != (Ft, B) or scores.shape[2] < 1:
        raise ValueError("still: scores must be float32 [F,B,C] (layout 'FBC' only)")
    C = scores.shape[2]
    if keep_idx.dtype != torch.int32 or keep_idx.dim() != 3 or tuple(keep_idx.shape[:2]) != (Ft, C) or keep_idx.shape[2] < 1:
        raise ValueError("still: keep_idx must be int32 [F,C,cap]")
    if keep_cnt.dtype != torch.int32 or tuple(keep_cnt.shape) != (Ft, C):
        raise ValueError("still: keep_cnt must be int32 [F,C]")
    return (boxes, scores, keep_idx, keep_cnt), B, C, keep_idx.shape[2]


def propagate_detections(motion, still, top, reach=3, decay=1.0, sync=True, ctx=None):
    """Motion-guided propagation: every frame's confident still-image detections copied to the ``reach`` frames on either side
    of it, moved along the motion of their pixels, so that a frame where the detector missed the object still holds a box before
    NMS and before tubelets are seeded (include/vdet_hip.h: vdet_propagate_boxes; the rule is tests/motion_spec.py).  One launch,
    no host wait.

    ``motion``: the dict of ``motion_field`` of the same video.  ``still`` = (boxes [F,B,4] f32, scores [F,B,C] f32, keep_idx
    [F,C,k] int32, keep_cnt [F,C] int32): NMS survivors as ``nms_tracks`` takes them ('FBC').  The sources are the first
    min(``top``, keep_cnt) entries of every list.  A box moves, step by step, by the mean vector (rounded half up) of the blocks
    whose centre lies in it; a box wholly outside the image, or the video's end, ends its chain.  ``decay`` multiplies the score
    once per step (f32); 1.0 keeps the source's bits.

    Returns a dict in the tubelet layout, T = 2*reach*top slots (slot di*top + j for the j-th source of the frame ``delta`` away,
    di enumerating delta = -reach..-1, 1..reach): ``tracks`` [C,T,F,5] f32 (the source's coordinates plus the shift, the score),
    ``score`` [C,T,F] f32, ``src`` [C,T,F] int32 (the source's box index; INT32_MIN where no chain arrives), ``ntracks`` [C]
    int32 (T) -- NaN where no chain arrives.  A keep count or index out of range, or a source box that is not finite or beyond
    2^20, raises ValueError when the call -- or with ``sync=False`` a later ``ctx.sync()`` -- waits; that source writes NaN rows.

        idx, cnt = nms_volume(boxes, scores, 0.3);  still = (boxes, scores, idx, cnt)
        m = motion_field(images)
        p = propagate_detections(m, still, top=100)
        dets = nms_tracks(p['tracks'], p['ntracks'], p['score'], still=still, thresh=0.3)

    and ``dets`` goes to ``DetEvaluator.add_detections``, or -- ``tracks`` / ``ntracks`` / ``score`` -- to ``top_anchors``.
    ValueError for arguments beyond the limits (1 <= top <= k, 1 <= reach <= 16, 2*reach*top <= 1024, C*T*F < 2^31 - 16, decay
    finite and >= 0), before any launch."""
    fsum, block, H, W, F, Hb, Wb = _pd_motion(motion)
    still, B, C, kcap = _pd_still(still, F)
    top, reach, decay = int(top), int(reach), float(decay)
    if not 1 <= top <= kcap:
        raise ValueError("top = %d; 1 .. the capacity of the keep lists (%d)" % (top, kcap))
    if not 1 <= reach <= _MOTION_MAX_REACH:
        raise ValueError("reach = %d; 1 .. %d" % (reach, _MOTION_MAX_REACH))
    T = 2 * reach * top
    if T > _TN_MAX:
        raise ValueError("2*reach*top = %d slots per class; the limit is %d" % (T, _TN_MAX))
    if not math.isfinite(decay) or decay < 0:
        raise ValueError("decay must be finite and >= 0")
    if C * T * F >= 2 ** 31 - 16:
        raise ValueError("too many tubelet boxes (C*T*F must stay below 2^31 - 16)")
    _same_gpu((fsum,) + tuple(still), "motion and still")
    boxes, scores, keep_idx, keep_cnt = (x.contiguous() for x in still)
    ctx = _ctx_for(fsum, ctx)
    dev = fsum.device
    tracks = torch.empty((C, T, F, 5), dtype=torch.float32, device=dev)
    score = torch.empty((C, T, F), dtype=torch.float32, device=dev)
    src = torch.empty((C, T, F), dtype=torch.int32, device=dev)
    ntracks = torch.empty((C,), dtype=torch.int32, device=dev)
    ctx.check(ctx.lib.vdet_propagate_boxes(ctx.h, fsum.data_ptr(), F, Hb, Wb, block, H, W, B, C, boxes.data_ptr(), scores.data_ptr(),
                                           keep_idx.data_ptr(), kcap, keep_cnt.data_ptr(), top, reach, decay, tracks.data_ptr(),
                                           score.data_ptr(), src.data_ptr(), ntracks.data_ptr()))
    if sync:
        ctx.sync()
    return dict(tracks=tracks, ntracks=ntracks, score=score, src=src)


def _context_videos(scores, frame_off, C=None):
    """(F, B, C, offsets or None) of a score volume [F,B,C] that the context stage reads, with its optional video split.  The
    stage has no boxes, so F and B are the scores' own (``_volume_layout`` takes them from the boxes)."""
    ss = tuple(getattr(scores, 'shape', ()))
    if getattr(scores, 'dtype', None) != torch.float32 or len(ss) != 3 or (C is not None and ss[2] != C):
        raise ValueError("scores must be float32 [F,B,C]" + ("" if C is None else " with C = %d" % C))
    if min(ss) < 1:
        raise ValueError("scores must hold at least one frame, one box per frame and one class")
    F, B, C = ss
    return F, B, C, None if frame_off is None else _frame_offsets(frame_off, F)


def context_classes(scores, ratio=0.0003, top=None, min_hits=1, score_thresh=None, frame_off=None, sync=True, ctx=None):
    """Multi-context suppression, first half: the classes a video's highest-ranked detection scores belong to (include/vdet_hip.h:
    vdet_context_classes; the rule is tests/context_spec.py, which the device matches on bits).  T-CNN runs the stage between
    the still-image detector and per-frame NMS / tubelet seeding; the reference library has no function for it.

    scores [F,B,C] f32, class innermost; ``frame_off`` [V+1] splits the frames into videos (as ``top_anchors``), every step
    then runs per video.  A candidate is a score that is not NaN and -- with ``score_thresh`` -- is > score_thresh (float32
    compare; ``-inf`` drops io.py's padding, without a threshold ``-inf`` IS a candidate); n is their number.  The rank is
    k = min(top, n) with ``top``, else max(1, floor(ratio * n)) clamped to n (one float64 product).  ``thresh`` is the k-th
    largest candidate (-0.0 == +0.0; +inf when n == 0), ``hits[c]`` the number of candidates of class c that are >= thresh
    (every tie counts), ``high[c]`` = hits[c] >= min_hits.

    ``ratio`` = 0.0003 (and ``suppress_context``'s penalty 0.4) are starting points recalled from the T-CNN paper: they are
    not taken from the reference and not tuned.

    Returns (thresh [V] f32, n [V] int64, hits [V,C] int32, high [V,C] bool); without ``frame_off`` the V axis is dropped.  No
    host wait with ``sync=False``.  ValueError -- before any launch -- for a wrong dtype, device or shape, ``ratio`` outside
    (0, 1], ``top`` < 1, ``min_hits`` < 1, and beyond the limits (F*B < 2^31 - 16, every video below 2^32 scores)."""
    ratio = float(ratio)
    if top is None and not 0.0 < ratio <= 1.0:
        raise ValueError("ratio must lie in (0, 1]")
    if top is not None and int(top) < 1:
        raise ValueError("top must be at least 1")
    if int(min_hits) < 1:
        raise ValueError("min_hits must be at least 1")
    F, B, C, off = _context_videos(scores, frame_off)
    _same_gpu((scores,), "scores")
    ctx = _ctx_for(scores, ctx)
    scores = scores.contiguous()
    lead = () if off is None else (len(off) - 1,)
    dev = scores.device
    thresh = torch.empty(lead, dtype=torch.float32, device=dev)
    n = torch.empty(lead, dtype=torch.int64, device=dev)
    hits = torch.empty(lead + (C,), dtype=torch.int32, device=dev)
    high = torch.empty(lead + (C,), dtype=torch.bool, device=dev)
    ctx.check(ctx.lib.vdet_context_classes(
        ctx.h, scores.data_ptr(), F, B, C, ratio, 0 if top is None else min(int(top), 2 ** 62), min(int(min_hits), 2 ** 62),
        0 if score_thresh is None else 1, 0.0 if score_thresh is None else float(score_thresh),
        off.ctypes.data if off is not None else None, 0 if off is None else len(off) - 1,
        thresh.data_ptr(), n.data_ptr(), hits.data_ptr(), high.data_ptr()))
    if sync:
        ctx.sync()
    return thresh, n, hits, high


def suppress_context(scores, high, penalty=0.4, frame_off=None, out=None, sync=True, ctx=None):
    """Multi-context suppression, second half: ``penalty`` (as a float32, one subtraction) off every score whose class is not
    among its video's high-confidence classes; scores of high classes and NaN are copied bit for bit, ``-inf`` stays ``-inf``
    (include/vdet_hip.h: vdet_suppress_context).  One launch, one read and one write.

    scores [F,B,C] f32; ``high`` bool [C], or [V,C] with ``frame_off`` [V+1]: ``context_classes``' last output.  ``out``: None
    allocates; ``out=scores`` works in place (a c2 volume is 2.4 GB); any other contiguous f32 tensor of the scores' shape on
    the same GPU that does not overlap them is written.  Returns the suppressed scores.  The default penalty is a starting
    point recalled from the T-CNN paper, not taken from the reference and not tuned.  ValueError before any launch for a wrong
    dtype, device or shape and for a penalty that is not finite (as a float32) or is < 0."""
    penalty = float(penalty)
    if not math.isfinite(penalty) or penalty < 0 or penalty > float(np.finfo(np.float32).max):
        raise ValueError("penalty must be finite (as a float32) and >= 0")
    F, B, C, off = _context_videos(scores, frame_off)
    if high.dtype != torch.bool or tuple(high.shape) != ((C,) if off is None else (len(off) - 1, C)):
        raise ValueError("high must be bool [C], or [V,C] with frame_off, for scores [F,B,%d]" % C)
    inplace = out is scores
    if out is not None and not inplace:
        if out.dtype != torch.float32 or out.shape != scores.shape or not out.is_contiguous():
            raise ValueError("out must be scores itself or a contiguous float32 tensor of the scores' shape")
    if inplace and not scores.is_contiguous():
        raise ValueError("out=scores needs contiguous scores")
    _same_gpu((scores, high, out), "scores, high and out")
    ctx = _ctx_for(scores, ctx)
    scores, high = scores.contiguous(), high.contiguous()
    if out is None:
        out = torch.empty_like(scores)
    elif inplace:
        out = scores
    ctx.check(ctx.lib.vdet_suppress_context(
        ctx.h, scores.data_ptr(), F, B, C, high.data_ptr(), penalty, off.ctypes.data if off is not None else None,
        0 if off is None else len(off) - 1, out.data_ptr()))
    if sync:
        ctx.sync()
    return out


def _rt_call(ctx, off, B, C, T, tracks, ntracks, boxes, scores, floor, overlap_thres, complete, window, sync):
    """The one call behind rescore_tubelets / rescore_tubelets_batch: flat tensors in, flat outputs back."""
    V, Ft = len(off) - 1, int(off[-1])
    if B > 32767:
        raise ValueError("B = %d boxes per frame; the limit is 32767" % B)
    if V > 65535:
        raise ValueError("at most 65535 videos in one call")
    if Ft * B > 0x7FFFFFF0 or C * max(T, 1) * Ft >= 0x7FFFFFF0:
        raise ValueError("volume too large (F*B and C*T*F must stay below 2^31 - 16)")
    dev = boxes.device
    n = C * T * Ft
    det = torch.empty((n,), dtype=torch.float64, device=dev)
    pooled = torch.empty((n,), dtype=torch.float64, device=dev)
    tboxes = torch.empty((n * 4,), dtype=torch.float32, device=dev)
    src = torch.empty((n,), dtype=torch.int32, device=dev)
    complete = floor is None if complete is None else bool(complete)
    tail = (B, C, T, tracks.data_ptr(), ntracks.data_ptr(), boxes.data_ptr(), scores.data_ptr(),
            floor.data_ptr() if floor is not None else None, int(floor is not None and floor.dtype == torch.float64),
            float(overlap_thres), int(complete), int(window), det.data_ptr(), pooled.data_ptr(), tboxes.data_ptr(), src.data_ptr())
    if V == 1:
        ctx.check(ctx.lib.vdet_rescore_tubelets(ctx.h, Ft, *tail))
    else:
        ctx.check(ctx.lib.vdet_rescore_tubelets_batch(ctx.h, off.ctypes.data, V, *tail))
    if sync:
        ctx.sync()
    return det, pooled, tboxes, src


def rescore_tubelets(tracks, ntracks, boxes, scores, floor=None, overlap_thres=0.7, window=3, complete=None, sync=True, ctx=None):
    """Re-score ANY tubelet set against the detections (include/vdet_hip.h: vdet_rescore_tubelets): ``rescore_tracks``' three
    steps -- spatial max-pooling (raw_dets_spatial_max_pooling, vdet/tubelet_cls.py:493-535), gap completion (:284-303),
    temporal max-pooling (:386-414) -- with a tubelet taken as the LIST of its boxes, as the reference takes it: holes (NaN
    rows) inside a tubelet are no list elements, so completion and the pool work on ordinals.  ``rescore_tracks`` is for
    ``track_volume``'s own contiguous tubelets; on those the two agree bit for bit.

    tracks [C,T,F,5] f32, ntracks [C] int32, boxes [F,B,4] / scores [F,B,C] f32.  ``floor`` [C,T,F] f32 or f64: a box's own
    score, kept unless an overlapping detection scores strictly higher (the half of rcnn_sampling_dets_scoring, :221-259, that
    follows the CNN); without it a miss scores -1e5.  ``complete``: run the gap completion (default: only without a floor).
    Returns (det f64 [C,T,F], pooled f64 [C,T,F], tboxes f32 [C,T,F,4], src int32 [C,T,F]: the winning detection or -1);
    NaN / -1 where there is no box.  IndexError for a tubelet whose every box misses under completion (at the call, or at a
    later ``ctx.sync()`` with ``sync=False``)."""
    if window % 2 != 1:
        raise ValueError('Window size must be odd!')
    C, T, F = _tubelets_layout(tracks, ntracks)
    if floor is not None and (floor.dtype not in _F32_F64 or tuple(floor.shape) != (C, T, F)):
        raise ValueError("floor must be float32 or float64 [C,T,F]")
    boxes, scores, F, B, C = _volume(boxes, scores, (tracks, ntracks, floor), "tracks, ntracks, boxes, scores and floor", F=F, C=C,
                                     nonempty=True)
    ctx = _ctx_for(boxes, ctx)
    off = np.array([0, F], dtype=np.int64)
    det, pooled, tboxes, src = _rt_call(ctx, off, B, C, T, tracks.contiguous(), ntracks.contiguous(), boxes, scores,
                                        None if floor is None else floor.contiguous(), overlap_thres, complete, window, sync)
    return det.view(C, T, F), pooled.view(C, T, F), tboxes.view(C, T, F, 4), src.view(C, T, F)


def rescore_tubelets_batch(batch_out, boxes, scores, floor=None, overlap_thres=0.7, window=3, complete=None, sync=True, ctx=None):
    """``rescore_tubelets`` for every video of ANY dict in ``video_batch``'s layout (``_batch_read``) in one call; boxes [F,B,4] /
    scores [F,B,C] f32 are the batch's volume.  ``floor``, f32 or f64: one flat tensor in the batch layout, or a list of
    per-video [C,T,F_v] tensors -- used in place when they are the layout's consecutive views, gathered into one buffer when
    not.  Per video the bits are ``rescore_tubelets``' on that video alone.  Returns a NEW dict in the same layout -- the
    input's ``tracks``, ``anchors``, ``ntracks`` and ``frame_off`` carried over, new ``det`` / ``pooled`` / ``tboxes`` / ``src``.
    The input dict is not modified."""
    if window % 2 != 1:
        raise ValueError('Window size must be odd!')
    b = _batch_read(batch_out)
    off, V, Ft, C, T, tracks, ntracks = b.off, b.V, b.Ft, b.C, b.T, b.tracks, b.ntracks
    _, B, _ = _volume_layout(boxes, scores, F=Ft, C=C, nonempty=True)
    if floor is not None:
        if isinstance(floor, (list, tuple)):
            floor = _batch_field(b, floor, 1, _F32_F64, 'floor', 'rescore_tubelets_batch', gather=True)
        if not torch.is_tensor(floor) or floor.numel() != C * T * Ft:
            raise ValueError("floor must hold C*T*F elements in the batch layout")
        if floor.dtype not in _F32_F64:
            raise ValueError("floor must be float32 or float64")
        floor = floor.contiguous()
    _same_gpu((boxes, scores, tracks, ntracks, floor), "the batch result, boxes, scores and floor")
    ctx = _ctx_for(boxes, ctx)
    det, pooled, tboxes, src = _rt_call(ctx, off, B, C, T, tracks, ntracks, boxes.contiguous(), scores.contiguous(), floor,
                                        overlap_thres, complete, window, sync)
    views = lambda flat, per: _batch_views(flat, off, C, T, per)
    out = dict(tracks=list(batch_out['tracks']), ntracks=batch_out['ntracks'], frame_off=off, det=views(det, 1),
               pooled=views(pooled, 1), tboxes=views(tboxes, 4), src=views(src, 1))
    if 'anchors' in batch_out:
        out['anchors'] = batch_out['anchors']
    return out


_PATCH_DTYPES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}     # include/vdet_hip.h: VDET_PATCH_F32 / _F16 / _BF16
_PATCH_MODES = {'warp': 0, 'square': 1}


def _patch_common(images, crop_size, padding, mean, mode, dtype):
    """The checks rcnn_patches and tubelet_patches share: (S, padding, mode code, dtype code, mean tensor or None)."""
    _images(images)
    if not images.is_cuda:
        raise ValueError("expected a CUDA/HIP tensor (vdetlib_amd has no CPU path)")
    S, padding = int(crop_size), int(padding)
    if not 1 <= S <= 1024:
        raise ValueError("crop_size = %d; 1 .. 1024" % S)
    if padding < 0 or S - 2 * padding < 1:
        raise ValueError("padding = %d; 0 <= padding and crop_size - 2*padding >= 1" % padding)
    if mode not in _PATCH_MODES:
        raise ValueError("mode must be 'warp' or 'square'")
    if dtype not in _PATCH_DTYPES:
        raise ValueError("dtype must be torch.float32, torch.float16 or torch.bfloat16")
    if mean is not None:
        if torch.is_tensor(mean):
            if mean.dtype != torch.float64 or tuple(mean.shape) != (3,) or mean.device != images.device:
                raise ValueError("mean must be three values, or a float64 [3] tensor on the images' GPU")
            mean = mean.contiguous()
        else:
            m = np.asarray(mean, dtype=np.float64).reshape(-1)
            if m.size != 3:
                raise ValueError("mean must be three values, or a float64 [3] tensor on the images' GPU")
            mean = torch.from_numpy(m).to(images.device)
    return S, padding, _PATCH_MODES[mode], _PATCH_DTYPES[dtype], mean


def _boxes_and_index(boxes, image_idx, Fi, single):
    """The box / image_idx checks rcnn_patches and roi_pool share -> N: boxes f32 / f64 [N,4], image_idx int32 [N] (None needs
    Fi == 1; ``single``: that layout, for the message), both contiguous."""
    if not torch.is_tensor(boxes) or boxes.dtype not in (torch.float32, torch.float64) or boxes.dim() != 2 or boxes.shape[1] != 4:
        raise ValueError("boxes must be float32 / float64 [N,4]")
    N = boxes.shape[0]
    if image_idx is None:
        if Fi != 1:
            raise ValueError("image_idx=None needs a single image (%s)" % single)
    elif not torch.is_tensor(image_idx) or image_idx.dtype != torch.int32 or tuple(image_idx.shape) != (N,):
        raise ValueError("image_idx must be int32 [N]")
    if not all(x is None or x.is_contiguous() for x in (boxes, image_idx)):
        raise ValueError("boxes and image_idx must be contiguous")
    return N


def _tubelet_range(tracks, ntracks, frames, cap, Fi, who):
    """The tubelet checks tubelet_patches and tubelet_rois share -> (C, T, F, ld, f0, f1, cap): tracks f32 / f64 [C,T,F,>=4],
    ntracks int32 [C], both contiguous; frames a range of the video that ``who`` (Fi entries) covers; cap a window count."""
    if not torch.is_tensor(tracks) or tracks.dtype not in (torch.float32, torch.float64) or tracks.dim() != 4 or tracks.shape[3] < 4:
        raise ValueError("tracks must be float32 / float64 [C,T,F,>=4]")
    C, T, F, ld = tracks.shape
    if C < 1 or F < 1:
        raise ValueError("at least one class and one frame")
    if not torch.is_tensor(ntracks) or ntracks.dtype != torch.int32 or tuple(ntracks.shape) != (C,):
        raise ValueError("ntracks must be int32 [C]")
    if C * max(T, 1) * F >= 2 ** 31 - 16:
        raise ValueError("too many tubelet boxes (C*T*F must stay below 2^31 - 16)")
    try:
        f0, f1 = (int(x) for x in frames)
    except (TypeError, ValueError):
        raise ValueError("frames must be (f0, f1)")
    if not 0 <= f0 < f1 <= F:
        raise ValueError("frames must be a range 0 <= f0 < f1 <= F (F = %d)" % F)
    if Fi != f1 - f0:
        raise ValueError("%s must hold the f1 - f0 = %d frames of the range" % (who, f1 - f0))
    cap = int(cap)
    if not 0 <= cap < 2 ** 31 - 16:
        raise ValueError("cap must be 0 .. 2^31 - 17 windows")
    if not tracks.is_contiguous() or not ntracks.is_contiguous():
        raise ValueError("tracks and ntracks must be contiguous")
    return C, T, F, ld, f0, f1, cap


def rcnn_patches(images, boxes, image_idx=None, offsets=None, crop_size=224, padding=16, mean=(103.939, 116.779, 123.68),
                 mode='warp', dtype=torch.float32, sync=True, ctx=None):
    """The CNN scorers' input windows on the device (include/vdet_hip.h: vdet_rcnn_patches): ``rcnn_img_crop`` +
    ``im_transform`` (utils/common.py:208-280) for every box in one launch -- context padding, Python-2 rounding, clipping,
    bilinear resize in f64, minus the mean, zero canvas, channel-major.

    images uint8 [Fi,H,W,3] in the stored channel order (BGR from cv2.imread: never swapped); boxes [N,4] f32 / f64, 1-based
    inclusive; image_idx int32 [N] (None: a single image).  ``offsets`` f64 [N,num,4] is ``sampling_boxes``
    (vdet/tubelet_cls.py:136-142) with the caller's draw: window (n,0) is box n, window (n,1+j) is
    box + offsets[n,j]*[w,h,w,h].  ``mean`` None: no subtraction.  ``mode`` 'warp' / 'square'.  ``dtype`` float32, or float16 /
    bfloat16: the f32 value rounded once (== patches_f32.to(dtype)).

    Returns a dict: ``patches`` [N,3,S,S] (with offsets [N,num+1,3,S,S]), ``ok`` uint8 [N] ([N,num+1]): 0 where the reference
    would raise inside cv2.resize (or the input is not finite, or the image index is out of range) -- that patch is all zeros --
    and with offsets ``sboxes`` f64 [N,num+1,4], the boxes used.  Parity of the resize rule with OpenCV is unpinned (DESIGN.md
    10j); the bits are those of tests/patch_spec.py.  No CPU fallback."""
    S, padding, mcode, dcode, mean = _patch_common(images, crop_size, padding, mean, mode, dtype)
    N = _boxes_and_index(boxes, image_idx, images.shape[0], "[1,H,W,3]")
    num = 0
    if offsets is not None:
        if not torch.is_tensor(offsets) or offsets.dtype != torch.float64 or offsets.dim() != 3 or offsets.shape[0] != N or offsets.shape[2] != 4:
            raise ValueError("offsets must be float64 [N,num,4]")
        num = offsets.shape[1]
        if not 1 <= num <= 255:
            raise ValueError("num = %d sampled boxes per box; 1 .. 255" % num)
    M = N * (num + 1)
    if M >= 2 ** 31 - 16:
        raise ValueError("too many windows (below 2^31 - 16)")
    if offsets is not None and not offsets.is_contiguous():
        raise ValueError("offsets must be contiguous")
    _same_gpu((images, boxes, image_idx, offsets), "images, boxes, image_idx and offsets")
    dev = images.device
    patches = torch.empty((M, 3, S, S), dtype=dtype, device=dev)
    ok = torch.empty((M,), dtype=torch.uint8, device=dev)
    sboxes = torch.empty((N, num + 1, 4), dtype=torch.float64, device=dev) if offsets is not None else None
    ctx = _ctx_for(images, ctx)
    ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None
    ctx.check(ctx.lib.vdet_rcnn_patches(ctx.h, images.data_ptr(), images.shape[0], images.shape[1], images.shape[2], ptr(boxes),
                                        int(boxes.dtype == torch.float64), N, ptr(image_idx), ptr(offsets), num, ptr(mean), S, padding,
                                        mcode, dcode, ptr(patches), ptr(ok), ptr(sboxes)))
    if sync:
        ctx.sync()
    if offsets is None:
        return dict(patches=patches, ok=ok)
    return dict(patches=patches.view(N, num + 1, 3, S, S), ok=ok.view(N, num + 1), sboxes=sboxes)


def tubelet_patches(images, tracks, ntracks, frames, cap, crop_size=224, padding=16, mean=(103.939, 116.779, 123.68), mode='warp',
                    dtype=torch.float32, sync=True, ctx=None):
    """``rcnn_patches`` for the tubelet boxes of the frames ``frames = (f0, f1)``, f0 <= f < f1, straight from device tubelets
    (include/vdet_hip.h: vdet_tubelet_patches): the input of ``rcnn_scoring`` (vdet/tubelet_cls.py:102-134) for those frames.

    tracks: any [C,T,F,>=4] f32 / f64 tensor whose first four columns are the box -- ``tracks``, ``tboxes``, one video of a
    batch; ntracks int32 [C]; images uint8 [f1-f0,H,W,3], images[f - f0] is frame f.  The PRESENT boxes (t < ntracks[c], x1 not
    NaN) are compacted in the order frames, classes, slots -- the order of the reference's frame loop.  Returns a dict:
    ``patches`` [cap,3,S,S], ``slot`` int32 [cap,3] rows (c,t,f), -1 behind the count, ``count`` int32 [1]: the TRUE number of
    present boxes, ``ok`` uint8 [cap].  ``count > cap`` raises ValueError when the call -- with ``sync=False`` a later
    ``ctx.sync()`` -- waits; the first ``cap`` windows are valid then.  The other options are ``rcnn_patches``'.

    The way back, with any torch ``net`` giving one score per patch::

        n = int(out['count']); c, t, f = out['slot'][:n].long().unbind(1)
        series = torch.full(tracks.shape[:3], float('nan'), dtype=torch.float64, device=tracks.device)
        series[c, t, f] = net(out['patches'][:n]).double()
        det, pooled, tboxes, src = rescore_tubelets(tracks, ntracks, boxes, scores, floor=series)"""
    S, padding, mcode, dcode, mean = _patch_common(images, crop_size, padding, mean, mode, dtype)
    C, T, F, ld, f0, f1, cap = _tubelet_range(tracks, ntracks, frames, cap, images.shape[0], "images")
    _same_gpu((images, tracks, ntracks), "images, tracks and ntracks")
    dev = images.device
    patches = torch.empty((cap, 3, S, S), dtype=dtype, device=dev)
    ok = torch.empty((cap,), dtype=torch.uint8, device=dev)
    slot = torch.empty((cap, 3), dtype=torch.int32, device=dev)
    count = torch.empty((1,), dtype=torch.int32, device=dev)
    ctx = _ctx_for(images, ctx)
    ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None
    ctx.check(ctx.lib.vdet_tubelet_patches(ctx.h, images.data_ptr(), images.shape[0], images.shape[1], images.shape[2], ptr(tracks),
                                           int(tracks.dtype == torch.float64), C, T, F, ld, ntracks.data_ptr(), f0, f1, cap, ptr(mean),
                                           S, padding, mcode, dcode, ptr(patches), ptr(ok), ptr(slot), count.data_ptr()))
    if sync:
        ctx.sync()
    return dict(patches=patches, slot=slot, count=count, ok=ok)


_ROI_MODES = {'max': 0, 'align': 1}       # include/vdet_hip.h: VDET_ROI_MAX / VDET_ROI_ALIGN


def _roi_common(features, spatial_scale, pooled, box_scale, mode, sampling):
    """The checks roi_pool and tubelet_rois share: (feature dtype code, spatial_scale, ph, pw, box_scale, mode code, sampling)."""
    if not torch.is_tensor(features) or features.dtype not in _PATCH_DTYPES or features.dim() != 4 or 0 in features.shape:
        raise ValueError("features must be float32 / float16 / bfloat16 [Fi,K,Hf,Wf] with no empty dimension")
    if not features.is_contiguous():
        raise ValueError("features must be contiguous NCHW (channels_last is not supported)")
    if not features.is_cuda:
        raise ValueError("expected a CUDA/HIP tensor (vdetlib_amd has no CPU path)")
    if features.shape[2] > 32767 or features.shape[3] > 32767:
        raise ValueError("feature maps of at most 32767 x 32767")
    try:
        ph, pw = (int(x) for x in pooled)
    except (TypeError, ValueError):
        raise ValueError("pooled must be (ph, pw)")
    if not (1 <= ph <= 32 and 1 <= pw <= 32):
        raise ValueError("pooled = (%d, %d); 1 .. 32 each" % (ph, pw))
    if mode not in _ROI_MODES:
        raise ValueError("mode must be 'max' or 'align'")
    sampling = int(sampling)
    if mode == 'align' and not 1 <= sampling <= 8:
        raise ValueError("sampling = %d; 1 .. 8 (the adaptive grid is not provided)" % sampling)
    spatial_scale, box_scale = float(spatial_scale), float(box_scale)
    if not (0.0 < float(np.float32(spatial_scale)) < float('inf')) or not np.isfinite(box_scale):
        raise ValueError("spatial_scale must be positive and finite, box_scale finite")
    return _PATCH_DTYPES[features.dtype], spatial_scale, ph, pw, box_scale, _ROI_MODES[mode], sampling


def roi_pool(features, boxes, image_idx=None, spatial_scale=1 / 16., pooled=(7, 7), box_scale=1.0, mode='max', sampling=2,
             aligned=False, sync=True, ctx=None):
    """RoI pooling on the device (include/vdet_hip.h: vdet_roi_pool): the front half of the Fast R-CNN route -- the backbone
    runs once per image and every box is pooled out of its feature map, all RoIs of the call in one launch.

    features f32 / f16 / bf16 [Fi,K,Hf,Wf], contiguous NCHW (anything else, channels_last included: ValueError); boxes [N,4]
    f32 / f64 as they are (no 1-based shift); image_idx int32 [N] (None: a single image).  A RoI is
    ``f32(f64(box) * box_scale)`` -- ``box_scale`` is the image resize factor of ``im_detect`` -- and ``spatial_scale`` maps
    it to cells.  ``pooled = (ph, pw)``, 1 .. 32 each.  ``mode='max'``: Caffe's ROIPoolingLayer forward (rounded cell box, f32
    bin edges, an empty bin is 0, NaN and -inf cells never win).  ``mode='align'``: RoIAlign with a fixed grid of
    ``sampling`` x ``sampling`` (1 .. 8) bilinear samples per bin, ``aligned`` the half-pixel shift.  Both rules are RESTATED
    from public code that was not at hand; the bits are those of tests/roipool_spec.py.

    Returns a dict: ``pooled`` [N,K,ph,pw] in features.dtype (the f32 value rounded once), ``ok`` uint8 [N]: 0 -- and an
    all-zero block -- where a RoI coordinate is not finite, exceeds 2^24 cells, or the image index is out of range.  A RoI
    wholly off the map is ok and all zeros.  N = 0 is legal; N*K*ph*pw may exceed 2^31.  No CPU fallback."""
    dcode, spatial_scale, ph, pw, box_scale, mcode, sampling = _roi_common(features, spatial_scale, pooled, box_scale, mode, sampling)
    N = _boxes_and_index(boxes, image_idx, features.shape[0], "[1,K,Hf,Wf]")
    if N >= 2 ** 31 - 16:
        raise ValueError("too many RoIs (below 2^31 - 16)")
    _same_gpu((features, boxes, image_idx), "features, boxes and image_idx")
    Fi, K, Hf, Wf = features.shape
    dev = features.device
    out = torch.empty((N, K, ph, pw), dtype=features.dtype, device=dev)
    ok = torch.empty((N,), dtype=torch.uint8, device=dev)
    ctx = _ctx_for(features, ctx)
    ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None
    ctx.check(ctx.lib.vdet_roi_pool(ctx.h, features.data_ptr(), dcode, Fi, K, Hf, Wf, ptr(boxes), int(boxes.dtype == torch.float64), N,
                                    ptr(image_idx), spatial_scale, ph, pw, box_scale, mcode, sampling, int(bool(aligned)), ptr(out),
                                    ptr(ok)))
    if sync:
        ctx.sync()
    return dict(pooled=out, ok=ok)


def tubelet_rois(features, tracks, ntracks, frames, cap, spatial_scale=1 / 16., pooled=(7, 7), box_scale=1.0, mode='max', sampling=2,
                 aligned=False, sync=True, ctx=None):
    """``roi_pool`` for the tubelet boxes of the frames ``frames = (f0, f1)``, f0 <= f < f1, straight from device tubelets
    (include/vdet_hip.h: vdet_tubelet_rois): the input of ``fast_rcnn_cls`` (vdet/tubelet_cls.py:53-76) for those frames.

    tracks, ntracks, cap, ``slot``, ``count`` and the order of the compacted boxes (frames, classes, slots; present: t <
    ntracks[c] and x1 not NaN) are ``tubelet_patches``'; features [f1-f0,K,Hf,Wf], features[f - f0] is frame f's map.
    Returns a dict: ``pooled`` [cap,K,ph,pw], ``slot`` int32 [cap,3] rows (c,t,f), -1 behind the count, ``count`` int32 [1]:
    the TRUE number of present boxes, ``ok`` uint8 [cap].  ``count > cap`` raises ValueError when the call -- with
    ``sync=False`` a later ``ctx.sync()`` -- waits; the first ``cap`` blocks are valid then.  The other options are
    ``roi_pool``'s.

    The round trip for a chunk of frames, with any torch ``backbone`` and ``head`` (one score per pooled block)::

        feats = backbone(images[f0:f1])                                   # [f1-f0,K,Hf,Wf], once per frame
        out = tubelet_rois(feats, tracks, ntracks, (f0, f1), cap)
        n = int(out['count']); c, t, f = out['slot'][:n].long().unbind(1)
        series[c, t, f] = head(out['pooled'][:n]).double()                # series [C,T,F] f64, NaN where nothing is scored
        det, pooled, tboxes, src = rescore_tubelets(tracks, ntracks, boxes, scores, floor=series)

    or, for the TCN, the head's feature rows scattered the same way into the [C,T,F,ch] tensor that
    ``tcn_tracks(wide={'feats': ...})`` reads."""
    dcode, spatial_scale, ph, pw, box_scale, mcode, sampling = _roi_common(features, spatial_scale, pooled, box_scale, mode, sampling)
    C, T, F, ld, f0, f1, cap = _tubelet_range(tracks, ntracks, frames, cap, features.shape[0], "features")
    _same_gpu((features, tracks, ntracks), "features, tracks and ntracks")
    Fi, K, Hf, Wf = features.shape
    dev = features.device
    out = torch.empty((cap, K, ph, pw), dtype=features.dtype, device=dev)
    ok = torch.empty((cap,), dtype=torch.uint8, device=dev)
    slot = torch.empty((cap, 3), dtype=torch.int32, device=dev)
    count = torch.empty((1,), dtype=torch.int32, device=dev)
    ctx = _ctx_for(features, ctx)
    ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None
    ctx.check(ctx.lib.vdet_tubelet_rois(ctx.h, features.data_ptr(), dcode, Fi, K, Hf, Wf, ptr(tracks), int(tracks.dtype == torch.float64),
                                        C, T, F, ld, ntracks.data_ptr(), f0, f1, cap, spatial_scale, ph, pw, box_scale, mcode, sampling,
                                        int(bool(aligned)), ptr(out), ptr(ok), ptr(slot), count.data_ptr()))
    if sync:
        ctx.sync()
    return dict(pooled=out, slot=slot, count=count, ok=ok)


_FEAT_DTYPES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2, torch.float64: 3}     # include/vdet_hip.h: VDET_FEAT_*


def _svm_model(model, dev):
    """W [K,M], B [M] or None as device tensors, the scale 20 / feat_norm_mean as numpy computes it, and whether that scale is
    'at most float32' for numpy's result type (a python float is; a float64 scalar or array is not)."""
    W, B, fnm = model['W'], model['B'], model['feat_norm_mean']
    if not torch.is_tensor(W):
        W = torch.from_numpy(np.ascontiguousarray(np.asarray(W))).to(dev)
    if B is not None and not torch.is_tensor(B):
        B = torch.from_numpy(np.ascontiguousarray(np.asarray(B))).to(dev)
    if torch.is_tensor(fnm):
        fnm = fnm.detach().cpu().numpy()
    scale = 20. / fnm
    if np.size(scale) != 1:
        raise ValueError("feat_norm_mean must be a scalar")
    small = isinstance(scale, float) and not isinstance(scale, np.floating) or np.asarray(scale).dtype in (np.float32, np.float16)
    if W.dim() != 2 or W.dtype not in (torch.float32, torch.float64):
        raise ValueError("W must be float32 / float64 [K,M]")
    if B is not None:
        if B.dtype not in (torch.float32, torch.float64) or B.numel() != W.shape[1] or (B.dim() > 1 and tuple(B.shape) != (1, W.shape[1])):
            raise ValueError("B must be float32 / float64 [M] (or [1,M])")
        B = B.reshape(-1)
    if not W.is_contiguous() or not (B is None or B.is_contiguous()):
        raise ValueError("W and B must be contiguous")
    _same_gpu((W, B), "features, W and B", dev)
    return W, B, float(np.asarray(scale).reshape(())), bool(small)


def svm_head(features, model, group=1, slot=None, count=None, shape=None, cols=None, sboxes=None, ok=None, out=None, sync=True,
             ctx=None):
    """The CNN scorers after the net, on the device (include/vdet_hip.h: vdet_svm_head): ``svm_scores`` (vdet/image_det.py:
    109-114) for the ONE class column each window needs, the max / argmax over the ``group`` windows of a box
    (rcnn_sampling_scoring, vdet/tubelet_cls.py:166-189) and the scatter into [C,T,F].

    features [N*group, K] (or [N*group,K,1,1]) f64 / f32 / f16 / bf16: window n*group + j is window j of box n.  ``model``: the
    ``svm_from_rcnn_model`` dict, ``W`` [K,M] and ``B`` [M] f64 / f32 as device tensors or numpy, ``feat_norm_mean`` a scalar.
    The compute dtype is numpy's result type: float32 when features, W, B and the scale 20 / feat_norm_mean are all at most
    float32 (a python-float feat_norm_mean counts as such, a float64 scalar does not), else float64.

    ``slot`` int32 [N,3] rows (c,t,f) and ``count`` int32 [1] as ``tubelet_patches`` returns them (count None: all N; rows behind
    it are not read); ``shape`` = (C,T,F), or taken from ``out``.  ``cols`` int32 [C]: the column of W of class c (default the
    identity, C <= M; for VID classes ``index_vdet_to_det[c+1] - 1``).  Without ``slot`` (the ``rcnn_patches`` route) every box
    is of the one class ``cols[0]`` and only the compact form is written.  ``sboxes`` f64 [N,group,4] and ``ok`` uint8
    [N*group] (any shape of that size) are the patch calls': a window with ok == 0 does not compete; a box with no window left
    scores NaN with arg -1 and is counted in ``nbad``.  ``out``: the dict of an earlier call -- its det / arg / tboxes are
    written in place at this call's slots only (frame ranges of one video).  ``out=None`` allocates them, NaN / -1.

    Returns a dict: ``det`` [C,T,F] (compute dtype), ``arg`` int32 [C,T,F], ``tboxes`` f64 [C,T,F,4] (None without sboxes) --
    with slot=None det / arg are None and tboxes is [N,4] --, the compact ``score`` [N] and ``arg_flat`` int32 [N] (NaN / -1
    behind count), ``nbad`` int32 [1].  The bits are those of tests/svm_spec.py.  A slot outside ``shape`` or a column outside W
    raises ValueError when the call -- with ``sync=False`` a later ``ctx.sync()`` -- waits; that box is skipped.  No CPU
    fallback."""
    if not torch.is_tensor(features) or features.dtype not in _FEAT_DTYPES:
        raise ValueError("features must be a float64 / float32 / float16 / bfloat16 tensor")
    if not features.is_cuda:
        raise ValueError("expected a CUDA/HIP tensor (vdetlib_amd has no CPU path)")
    if features.dim() == 4 and features.shape[2] == 1 and features.shape[3] == 1:
        features = features[:, :, 0, 0]
    if features.dim() != 2 or features.shape[1] < 1:
        raise ValueError("features must be [N*group, K] with K >= 1")
    if not features.is_contiguous():
        raise ValueError("features must be contiguous")
    dev = features.device
    W, B, scale, small = _svm_model(model, dev)
    Mw, K = features.shape
    if W.shape[0] != K:
        raise ValueError("shapes %s and %s not aligned" % (tuple(features.shape), tuple(W.shape)))
    M = W.shape[1]
    G = int(group)
    if G < 1 or Mw % G:
        raise ValueError("group = %d windows per box must divide the %d feature rows" % (G, Mw))
    N = Mw // G
    f32 = features.dtype != torch.float64 and W.dtype == torch.float32 and small and (B is None or B.dtype == torch.float32)
    cdt = torch.float32 if f32 else torch.float64
    if f32:
        scale = float(np.float32(scale))
    if out is not None and slot is None:
        raise ValueError("out= needs slot")
    if slot is not None:
        if not torch.is_tensor(slot) or slot.dtype != torch.int32 or tuple(slot.shape) != (N, 3):
            raise ValueError("slot must be int32 [N,3]")
        if out is not None:
            if not isinstance(out, dict) or not torch.is_tensor(out.get('det')) or not torch.is_tensor(out.get('arg')):
                raise ValueError("out must be the dict of an earlier svm_head call")
            if shape is not None and tuple(shape) != tuple(out['det'].shape):
                raise ValueError("shape differs from out's")
            shape = tuple(out['det'].shape)
        try:
            C, T, F = (int(x) for x in shape)
        except (TypeError, ValueError):
            raise ValueError("shape must be (C, T, F)")
        if C < 1 or T < 1 or F < 1 or C * T * F >= 2 ** 31 - 16:
            raise ValueError("shape must be C, T, F >= 1 with C*T*F below 2^31 - 16")
    else:
        if count is not None or shape is not None:
            raise ValueError("count and shape need slot")
        C, T, F = 1, 1, 1
    if count is not None and (not torch.is_tensor(count) or count.dtype != torch.int32 or count.numel() != 1):
        raise ValueError("count must be int32 [1]")
    if cols is None:
        if C > M:
            raise ValueError("the identity cols needs C <= M columns of W")
    elif not torch.is_tensor(cols) or cols.dtype != torch.int32 or tuple(cols.shape) != (C,):
        raise ValueError("cols must be int32 [C]")
    if sboxes is not None and (not torch.is_tensor(sboxes) or sboxes.dtype != torch.float64 or tuple(sboxes.shape) != (N, G, 4)):
        raise ValueError("sboxes must be float64 [N,group,4]")
    if ok is not None and (not torch.is_tensor(ok) or ok.dtype != torch.uint8 or ok.numel() != N * G):
        raise ValueError("ok must be uint8 with N*group elements")
    if not all(x is None or x.is_contiguous() for x in (slot, count, cols, sboxes, ok)):
        raise ValueError("slot, count, cols, sboxes and ok must be contiguous")
    _same_gpu((slot, count, cols, sboxes, ok), "features, slot, count, cols, sboxes and ok", dev)
    det = arg = tboxes = None
    if slot is not None:
        if out is not None:
            det, arg, tboxes = out['det'], out['arg'], out.get('tboxes')
            if det.dtype != cdt or arg.dtype != torch.int32 or tuple(arg.shape) != (C, T, F):
                raise ValueError("out's det / arg do not fit this call (compute dtype %s, shape %s)" % (cdt, (C, T, F)))
            if sboxes is not None and (not torch.is_tensor(tboxes) or tboxes.dtype != torch.float64 or tuple(tboxes.shape) != (C, T, F, 4)):
                raise ValueError("out's tboxes must be float64 [C,T,F,4] when sboxes are given")
            if not all(x is None or x.is_contiguous() for x in (det, arg, tboxes)):
                raise ValueError("out's tensors must be contiguous on the features' GPU")
            _same_gpu((det, arg, tboxes), "features and out's tensors", dev)
        else:
            det = torch.full((C, T, F), float('nan'), dtype=cdt, device=dev)
            arg = torch.full((C, T, F), -1, dtype=torch.int32, device=dev)
            tboxes = torch.full((C, T, F, 4), float('nan'), dtype=torch.float64, device=dev) if sboxes is not None else None
    elif sboxes is not None:
        tboxes = torch.empty((N, 4), dtype=torch.float64, device=dev)
    score = torch.empty((N,), dtype=cdt, device=dev)
    arg_flat = torch.empty((N,), dtype=torch.int32, device=dev)
    nbad = torch.empty((1,), dtype=torch.int32, device=dev)
    ctx = _ctx_for(features, ctx)
    ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None
    ctx.check(ctx.lib.vdet_svm_head(ctx.h, ptr(features), _FEAT_DTYPES[features.dtype], N, G, K, W.data_ptr(),
                                    int(W.dtype == torch.float64), ptr(B), int(B is not None and B.dtype == torch.float64), M, scale,
                                    int(not f32), ptr(slot), ptr(count), C, T, F, ptr(cols), ptr(sboxes), ptr(ok), ptr(det), ptr(arg),
                                    ptr(tboxes) if sboxes is not None else None, ptr(score), ptr(arg_flat), nbad.data_ptr()))
    if sync:
        ctx.sync()
    return dict(det=det, arg=arg, tboxes=tboxes, score=score, arg_flat=arg_flat, nbad=nbad)


def svm_scores(features, model, sync=True, ctx=None):
    """``image_det.svm_scores`` (vdet/image_det.py:109-114) on DEVICE tensors, all M columns (include/vdet_hip.h:
    vdet_svm_scores_dev_f64 / _f32, the MFMA kernel of the host form): for the ``all_score`` rows of the CNN scorers -- gather
    the winners' feature rows by ``svm_head``'s ``arg`` and pass them in.  features [n,K] f64 / f32 on the GPU, ``model`` as for
    ``svm_head``.  The scaling ``features * (20 / feat_norm_mean)`` and the dtype rules are the host form's (torch's
    elementwise product stands in for numpy's, the same bits); B joins in the product's dtype.  Returns [n,M]."""
    if not torch.is_tensor(features) or features.dtype not in (torch.float32, torch.float64):
        raise ValueError("features must be a float64 / float32 tensor")
    if not features.is_cuda:
        raise ValueError("expected a CUDA/HIP tensor (vdetlib_amd has no CPU path)")
    if features.dim() == 4 and features.shape[2] == 1 and features.shape[3] == 1:
        features = features[:, :, 0, 0]
    if features.dim() != 2:
        raise ValueError("features must be [n, K]")
    dev = features.device
    W, B, scale, small = _svm_model(model, dev)
    if W.shape[0] != features.shape[1]:
        raise ValueError("shapes %s and %s not aligned" % (tuple(features.shape), tuple(W.shape)))
    f32 = features.dtype == torch.float32 and W.dtype == torch.float32 and small
    cdt = torch.float32 if f32 else torch.float64
    if B is not None and B.dtype == torch.float64 and f32:
        raise ValueError("a float64 B on a float32 product: use image_det.svm_scores (numpy promotes the sum)")
    a = (features if small else features.double()) * scale        # rounded in the features' dtype first, as numpy does (:112)
    a = a.to(cdt).contiguous()
    w = W.to(cdt).contiguous()
    b = None if B is None else B.to(cdt).contiguous()
    n, K = a.shape
    M = w.shape[1]
    out_t = torch.empty((n, M), dtype=cdt, device=dev)
    ctx = _ctx_for(features, ctx)
    fn = ctx.lib.vdet_svm_scores_dev_f32 if f32 else ctx.lib.vdet_svm_scores_dev_f64
    ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None
    ctx.check(fn(ctx.h, ptr(a), n, K, ptr(w), ptr(b), M, ptr(out_t)))
    if sync:
        ctx.sync()
    return out_t


def _evaluator_of(gt):
    return gt if isinstance(gt, DetEvaluator) else DetEvaluator(gt)


def tubelets_overlap(gt, video, tracks, ntracks, boxes=None, sync=True, ctx=None):
    """``tubelets_overlap`` (utils/protocol.py:467-489) on device tubelets, against the ground truth a ``DetEvaluator``
    holds on the device (``gt``: the evaluator -- both then share one copy of the table -- or a gt_table dict, which is
    uploaded for this call).  tracks [C,T,F,5] f32 (column c = class c + 1), ntracks [C] int32, boxes [C,T,F,4] f32 to
    measure instead of the track rows (rescore_tracks' boxes).  The f32 coordinates are used as they are (no int()
    truncation, see include/vdet_hip.h).  Returns (gt_overlap [C,T,F] f64, NaN where no box; mean_iou [C,T] f64;
    gt [C,T] int32 flags)."""
    ev = _evaluator_of(gt)
    if tracks.dtype != torch.float32 or tracks.dim() != 4 or tracks.shape[3] != 5:
        raise ValueError("tracks must be float32 [C,T,F,5]")
    C, T, F = tracks.shape[0], tracks.shape[1], tracks.shape[2]
    if ntracks.dtype != torch.int32 or tuple(ntracks.shape) != (C,):
        raise ValueError("ntracks must be int32 [C]")
    if boxes is not None and (boxes.dtype != torch.float32 or tuple(boxes.shape) != (C, T, F, 4)):
        raise ValueError("boxes must be float32 [C,T,F,4]")
    if F < 1:
        raise ValueError("a video needs at least one frame")
    ev._check(tracks, ntracks, *([boxes] if boxes is not None else []))
    tracks, ntracks = tracks.contiguous(), ntracks.contiguous()
    boxes = None if boxes is None else boxes.contiguous()
    dev = tracks.device
    ov = torch.empty((C, T, F), dtype=torch.float64, device=dev)
    mean = torch.empty((C, T), dtype=torch.float64, device=dev)
    flag = torch.empty((C, T), dtype=torch.int32, device=dev)
    slots = ev._col_slots(C, 1)
    ctx = _ctx_for(tracks, ctx)
    gtb, gto, gtm, K = ev.device_table()
    ctx.check(ctx.lib.vdet_tubelets_overlap(
        ctx.h, gtb.data_ptr(), gto.data_ptr(), gtm.data_ptr(), K, ev._vidx.get(video, -1), F, C, T, tracks.data_ptr(),
        boxes.data_ptr() if boxes is not None else None, ntracks.data_ptr(), slots.ctypes.data, ov.data_ptr(), mean.data_ptr(),
        flag.data_ptr()))
    if sync:
        ctx.sync()
    return ov, mean, flag


def tubelets_overlap_batch(gt, videos, batch_out, use_tboxes=False, sync=True, ctx=None):
    """``tubelets_overlap`` for every video of a dict in ``video_batch``'s layout (``_batch_read``) in one launch.  Returns
    (gt_overlap: flat f64 buffer in the batch layout -- what ``tcn_tracks_batch`` takes --, its per-video [C,T,F_v] views,
    mean_iou [V,C,T], gt [V,C,T])."""
    ev = _evaluator_of(gt)
    b = _batch_read(batch_out)
    off, V, Ft, C, T, tracks, ntracks = b.off, b.V, b.Ft, b.C, b.T, b.tracks, b.ntracks
    if len(videos) != V:
        raise ValueError("one name per video of the batch")
    boxes = None
    if use_tboxes:
        if not batch_out.get('tboxes'):
            raise ValueError("video_batch ran without re-scoring (rescore=False): no tboxes")
        boxes = _batch_field(b, batch_out['tboxes'], 4, _F32, 'tboxes', 'batch_out')
    ev._check(tracks, ntracks, *([boxes] if boxes is not None else []))
    dev = tracks.device
    ov = torch.empty((C * T * Ft,), dtype=torch.float64, device=dev)
    mean = torch.empty((V, C, T), dtype=torch.float64, device=dev)
    flag = torch.empty((V, C, T), dtype=torch.int32, device=dev)
    slots = ev._col_slots(C, 1)
    vids = np.array([ev._vidx.get(v, -1) for v in videos], dtype=np.int32)
    ctx = _ctx_for(tracks, ctx)
    gtb, gto, gtm, K = ev.device_table()
    ctx.check(ctx.lib.vdet_tubelets_overlap_batch(
        ctx.h, gtb.data_ptr(), gto.data_ptr(), gtm.data_ptr(), K, vids.ctypes.data, off.ctypes.data, V, C, T, tracks.data_ptr(),
        boxes.data_ptr() if boxes is not None else None, ntracks.data_ptr(), slots.ctypes.data, ov.data_ptr(), mean.data_ptr(),
        flag.data_ptr()))
    if sync:
        ctx.sync()
    return ov, _batch_views(ov, off, C, T, 1), mean, flag


class DetEvaluator(object):
    """Per-class AP / mAP of device detections (include/vdet_hip.h: the device evaluator); ``vdetlib_amd.eval.evaluate``
    is the specification -- same matching bit for bit, the same AP up to the order of one f64 sum (< 1e-12).

      ev = DetEvaluator(eval.gt_table_from_annots(annots), classes=None, iou_thr=0.5, rule='voc')
      ev.add_tracks(video, tracks, ntracks, scores, boxes=None)      # track_volume / rescore_tracks outputs
      ev.add_keep_lists(video, boxes, scores, keep_idx, keep_cnt)    # nms_volume[_topk] / nms_track_volume survivors
      ev.add_batch(videos, video_batch(...))                         # all videos of a batch, one match launch
      ev.add_detections(video, nms_tracks(...))                      # per-frame detections (or videos, nms_tracks_batch(...))
      aps, mAP = ev.compute()                                        # {class_index: AP}, float

    Every add appends its matched detections to a device stream of (class, score, tp); ``compute`` sorts it stably by
    (class, score desc), so detections of equal score keep the order of the adds -- the order in which the host
    evaluator would have to be given the videos.  ``compute(group=...)`` all-gathers the streams of every rank first
    (rank-major), so each rank builds its evaluator from the FULL ground-truth table and all ranks get the same mAP."""

    def __init__(self, gt_table, classes=None, iou_thr=0.5, rule='voc', device=None):
        if rule not in ('voc', 'ilsvrc'):
            raise ValueError("rule must be 'voc' or 'ilsvrc'")
        self.rule, self.iou_thr = rule, float(iou_thr)
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != 'cuda':
            raise ValueError("expected a CUDA/HIP device (vdetlib_amd has no CPU path)")
        vid = np.ascontiguousarray(gt_table['video'], dtype=np.int32).reshape(-1)
        frame = np.ascontiguousarray(gt_table['frame'], dtype=np.int64).reshape(-1)
        cls = np.asarray(gt_table['class_index'], dtype=np.int64).reshape(-1)
        bbox = np.ascontiguousarray(gt_table['bbox'], dtype=np.float64).reshape(-1, 4)
        if not (len(vid) == len(frame) == len(cls) == len(bbox)):
            raise ValueError("gt_table arrays differ in length")
        self.videos = list(gt_table['videos'])
        self._vidx = {v: i for i, v in enumerate(self.videos)}
        self.classes = sorted(set(int(c) for c in cls)) if classes is None else [int(c) for c in classes]
        if not self.classes:
            raise ValueError("no classes to evaluate")
        self._slot = {c: k for k, c in enumerate(self.classes)}
        K = len(self.classes)
        slot = np.array([self._slot.get(int(c), -1) for c in cls], dtype=np.int32)
        self.n_gt = np.bincount(slot[slot >= 0], minlength=K).astype(np.int64)
        NV = len(self.videos)
        nf = np.zeros(max(NV, 1), dtype=np.int64)
        ok = (slot >= 0) & (frame >= 0) & (vid >= 0) & (vid < NV)
        if ok.any():
            np.maximum.at(nf, vid[ok], frame[ok] + 1)
        nf = nf[:NV]
        ncell = int(nf.sum()) * K
        if ncell >= 2 ** 31 - 16:
            raise ValueError("ground-truth table too large (videos x frames x classes >= 2^31)")
        dev = self.device
        self._gt_boxes = torch.empty((max(len(bbox), 1), 4), dtype=torch.float64, device=dev)
        self._gt_off = torch.empty((ncell + 1,), dtype=torch.int32, device=dev)
        self._gt_meta = torch.empty((max(NV, 1), 2), dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            ctx = _ctx_for(self._gt_off, None)
            ctx.check(ctx.lib.vdet_eval_gt_upload(
                ctx.h, vid.ctypes.data, frame.ctypes.data, slot.ctypes.data, bbox.ctypes.data, len(vid), nf.ctypes.data, NV, K,
                self._gt_boxes.data_ptr(), self._gt_off.data_ptr(), self._gt_meta.data_ptr()))
        self._ngt = torch.from_numpy(self.n_gt).to(dev)
        self._cls_t = torch.tensor(self.classes, dtype=torch.int64, device=dev)
        self._n = 0
        self._st = (torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.float64, device=dev),
                    torch.empty(0, dtype=torch.uint8, device=dev))

    # -- stream ------------------------------------------------------------------------------------------------------
    def _reserve(self, extra):
        need = self._n + int(extra)
        if need <= self._st[0].numel():
            return
        cap = max(need, 2 * self._st[0].numel(), 1024)
        new = tuple(torch.empty(cap, dtype=t.dtype, device=self.device) for t in self._st)
        for a, b in zip(new, self._st):
            a[:self._n] = b[:self._n]
        self._st = new

    def _gt_args(self):
        return (self._gt_boxes.data_ptr(), self._gt_off.data_ptr(), self._gt_meta.data_ptr(), len(self.classes),
                0 if self.rule == 'voc' else 1, self.iou_thr)

    def device_table(self):
        """The uploaded ground-truth CSR (gt_boxes [G,4] f64, gt_off int32, vid_meta [NV,2] int64 device tensors, K class
        slots): shared with ``ops.tubelets_overlap`` so that the table lives on the device once."""
        return self._gt_boxes, self._gt_off, self._gt_meta, len(self.classes)

    def _col_slots(self, C, class_base):
        return np.array([self._slot.get(c + class_base, -1) for c in range(C)], dtype=np.int32)

    def _append(self, call, extra):
        self._reserve(extra)
        cnt = ctypes.c_int64(0)
        st = self._st
        with torch.cuda.device(self.device):
            ctx = _ctx_for(st[0], None)
            ctx.check(call(ctx, (st[0].data_ptr(), st[1].data_ptr(), st[2].data_ptr(), self._n, st[0].numel(), ctypes.byref(cnt))))
            ctx.sync()          # latched failures (a keep list out of order) surface here, before the stream grows
        self._n += int(cnt.value)
        return int(cnt.value)

    def _check(self, *ts):
        _same_gpu(ts, "the evaluator (%s) and every tensor" % self.device, self.device)

    def add_tracks(self, video, tracks, ntracks, scores, boxes=None):
        """Tubelets of one video: tracks [C,T,F,5] f32 (track_volume), ntracks [C] int32, scores [C,T,F] f64 or f32
        (NaN = no box; e.g. rescore_tracks' pooled), boxes [C,T,F,4] f32 (rescore_tracks' boxes; default: the track
        boxes).  Returns the number of detections added."""
        if tracks.dtype != torch.float32 or tracks.dim() != 4 or tracks.shape[3] != 5:
            raise ValueError("tracks must be float32 [C,T,F,5]")
        C, T, F = tracks.shape[0], tracks.shape[1], tracks.shape[2]
        if ntracks.dtype != torch.int32 or tuple(ntracks.shape) != (C,):
            raise ValueError("ntracks must be int32 [C]")
        if scores.dtype not in (torch.float32, torch.float64) or tuple(scores.shape) != (C, T, F):
            raise ValueError("scores must be float32 / float64 [C,T,F]")
        if boxes is not None and (boxes.dtype != torch.float32 or tuple(boxes.shape) != (C, T, F, 4)):
            raise ValueError("boxes must be float32 [C,T,F,4]")
        self._check(tracks, ntracks, scores, *([boxes] if boxes is not None else []))
        bx = (tracks if boxes is None else boxes).contiguous()
        scores, ntracks = scores.contiguous(), ntracks.contiguous()
        slots = self._col_slots(C, 1)
        vid = self._vidx.get(video, -1)
        stride = 5 if boxes is None else 4
        return self._append(lambda ctx, st: ctx.lib.vdet_eval_match_tracks(
            ctx.h, *self._gt_args(), vid, F, C, T, bx.data_ptr(), stride, scores.data_ptr(), int(scores.dtype == torch.float64),
            ntracks.data_ptr(), slots.ctypes.data, *st), C * T * F)

    def add_keep_lists(self, video, boxes, scores, keep_idx, keep_cnt, layout='FBC', class_base=1):
        """NMS survivors of one video: boxes [F,B,4] f32, scores [F,B,C] ('FBC') / [F,C,B] ('FCB') f32, keep_idx
        [F,C,cap] int32 (descending score: a list that is not, or a kept NaN score, raises ValueError), keep_cnt [F,C]
        int32; column c is class c + class_base.  Returns the number of detections added."""
        if boxes.dtype != torch.float32 or scores.dtype != torch.float32:
            raise ValueError("Buffer dtype mismatch, expected 'float32_t'")
        if keep_idx.dtype != torch.int32 or keep_cnt.dtype != torch.int32 or keep_idx.dim() != 3:
            raise ValueError("keep_idx must be int32 [F,C,cap], keep_cnt int32 [F,C]")
        F, C, cap = keep_idx.shape
        if boxes.dim() != 3 or boxes.shape[0] != F or boxes.shape[2] != 4 or tuple(keep_cnt.shape) != (F, C):
            raise ValueError("boxes [F,B,4], keep_idx [F,C,cap], keep_cnt [F,C]")
        B = boxes.shape[1]
        if layout == 'FBC':
            lay, shp = _lib.LAYOUT_FBC, (F, B, C)
        elif layout == 'FCB':
            lay, shp = _lib.LAYOUT_FCB, (F, C, B)
        else:
            raise ValueError("layout must be 'FBC' or 'FCB'")
        if tuple(scores.shape) != shp:
            raise ValueError("scores must be %s" % ('[F,B,C]' if layout == 'FBC' else '[F,C,B]'))
        self._check(boxes, scores, keep_idx, keep_cnt)
        boxes, scores, keep_idx, keep_cnt = boxes.contiguous(), scores.contiguous(), keep_idx.contiguous(), keep_cnt.contiguous()
        slots = self._col_slots(C, int(class_base))
        vid = self._vidx.get(video, -1)
        return self._append(lambda ctx, st: ctx.lib.vdet_eval_match_keep(
            ctx.h, *self._gt_args(), vid, boxes.data_ptr(), scores.data_ptr(), lay, F, B, C, keep_idx.data_ptr(),
            keep_cnt.data_ptr(), cap, slots.ctypes.data, *st), F * C * cap)

    def add_batch(self, videos, batch_out):
        """The re-scored tubelets (``pooled`` scores, ``tboxes`` boxes) of every video of a dict in ``video_batch``'s layout
        (``_batch_read``), in ONE match launch; videos[v] names video v.  Same stream as add_tracks video after video."""
        b = _batch_read(batch_out)
        if len(videos) != b.V:
            raise ValueError("one name per video of the batch")
        if not batch_out.get('pooled'):
            raise ValueError("video_batch ran without re-scoring (rescore=False): no tubelet scores")
        sc = _batch_field(b, batch_out['pooled'], 1, _F64, 'pooled', 'batch_out')
        bx = _batch_field(b, batch_out.get('tboxes'), 4, _F32, 'tboxes', 'batch_out')
        return self._append_batch(videos, b, bx, 4, sc)

    def _append_batch(self, videos, b, bx, stride, sc):
        """One match launch over the flat boxes ``bx`` (``stride`` floats per box) and f64 scores ``sc`` of the batch ``b``."""
        self._check(b.ntracks, sc, bx)
        vids = np.array([self._vidx.get(v, -1) for v in videos], dtype=np.int32)
        slots = self._col_slots(b.C, 1)
        return self._append(lambda ctx, st: ctx.lib.vdet_eval_match_tracks_batch(
            ctx.h, *self._gt_args(), vids.ctypes.data, b.off.ctypes.data, b.V, b.C, b.T, bx.data_ptr(), stride, sc.data_ptr(), 1,
            b.ntracks.data_ptr(), slots.ctypes.data, *st), b.C * b.T * b.Ft)

    def add_detections(self, video_or_videos, out):
        """The per-frame detections ``nms_tracks`` (``video_or_videos``: the video's name) or ``nms_tracks_batch`` (the names of
        the batch's videos; a dict in ``video_batch``'s layout, ``_batch_read``, checked like every other) returned: rows
        ``tracks[..., :4]`` scored by the f64 ``score``, rank as the slot axis.  Same stream as ``add_tracks`` of those arrays
        video after video; returns the number of detections added."""
        if not isinstance(out, dict) or any(k not in out for k in ('tracks', 'score', 'ntracks')):
            raise ValueError("out must be the dict nms_tracks or nms_tracks_batch returned")
        if 'frame_off' not in out:
            tr, sc, nt = out['tracks'], out['score'], out['ntracks']
            if tr.dtype != torch.float32 or tr.dim() != 4 or tr.shape[3] != 5:
                raise ValueError("tracks must be float32 [C,R,F,5]")
            C, R, F = tr.shape[0], tr.shape[1], tr.shape[2]
            if sc.dtype != torch.float64 or tuple(sc.shape) != (C, R, F) or nt.dtype != torch.int32 or tuple(nt.shape) != (C,):
                raise ValueError("score must be float64 [C,R,F], ntracks int32 [C]")
            self._check(tr, sc, nt)
            tr, sc, nt = tr.contiguous(), sc.contiguous(), nt.contiguous()
            slots, vid = self._col_slots(C, 1), self._vidx.get(video_or_videos, -1)
            return self._append(lambda ctx, st: ctx.lib.vdet_eval_match_tracks(
                ctx.h, *self._gt_args(), vid, F, C, R, tr.data_ptr(), 5, sc.data_ptr(), 1, nt.data_ptr(), slots.ctypes.data, *st),
                C * R * F)
        b = _batch_read(out, 'out')
        if isinstance(video_or_videos, str) or len(video_or_videos) != b.V:
            raise ValueError("one name per video of the batch")
        return self._append_batch(video_or_videos, b, b.tracks, 5, _batch_field(b, out['score'], 1, _F64, 'score', 'out'))

    def stream(self, raw=False):
        """The stream so far: (class_index int64, score f64, tp bool) device tensors (raw: class slot int32, tp uint8)."""
        s, sc, tp = (t[:self._n] for t in self._st)
        if raw:
            return s, sc, tp
        return self._cls_t[s.long()], sc, tp.bool()

    def compute(self, group=None, return_order=False):
        """({class_index: AP}, mAP over the classes with ground truth) -- eval.evaluate's result.  With ``group`` (or an
        initialised torch.distributed world) the streams of all ranks are gathered first (dist.gather_eval_stream)."""
        from . import dist as vdist
        s, sc, tp = vdist.gather_eval_stream(*self.stream(raw=True), group=group)
        n, K = s.numel(), len(self.classes)
        ap = torch.empty(K, dtype=torch.float64, device=self.device)
        perm = torch.empty(max(n, 1), dtype=torch.int32, device=self.device) if return_order else None
        s, sc, tp = s.contiguous(), sc.contiguous(), tp.contiguous()
        with torch.cuda.device(self.device):
            ctx = _ctx_for(ap, None)
            ctx.check(ctx.lib.vdet_eval_ap(ctx.h, s.data_ptr(), sc.data_ptr(), tp.data_ptr(), n, K, self._ngt.data_ptr(),
                                           ap.data_ptr(), perm.data_ptr() if perm is not None else None))
            ctx.sync()
        v = ap.cpu().numpy()
        aps = {c: float(v[k]) for k, c in enumerate(self.classes)}
        valid = [x for x in aps.values() if not np.isnan(x)]
        res = (aps, float(np.mean(valid)) if valid else float('nan'))
        if return_order:
            return res + ((self._cls_t[s.long()], sc, tp.bool(), perm[:n].long()),)
        return res
