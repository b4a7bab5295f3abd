"""Helpers of the reference's utils/common.py that the hot path and its callers use:
``iou`` (:451-468, computed on the GPU), ``options`` (:470-471), path/list helpers.

``rcnn_img_crop`` (:208-266) and ``im_transform`` (:268-280, the ``size <= 0`` branch) -- the window warp in front of the CNN
scorers -- run on the GPU (``ops.rcnn_patches``).

Out of scope (see DESIGN.md sections 7 and 10j): ``img_crop`` (:141-205, a uint8 imresize without a caller in the
reference), ``im_transform``'s resizing branch, MATLAB and Caffe launchers (:302-396), window files (:48-121).
"""
import argparse
import codecs
import os
import pickle as _pickle
import re
import tempfile


class AttrDict(dict):
    """Stand-in for easydict.EasyDict (not installed here): dict with attribute access, nested
    dicts converted recursively.  ``hasattr(opts, 'nms_thres')`` works as vdet/track.py expects."""

    def __init__(self, d=None, **kwargs):
        super(AttrDict, self).__init__()
        merged = dict(d or {})
        merged.update(kwargs)
        for k, v in merged.items():
            self[k] = v

    @staticmethod
    def _wrap(v):
        if isinstance(v, dict) and not isinstance(v, AttrDict):
            return AttrDict(v)
        if isinstance(v, (list, tuple)):
            return type(v)(AttrDict._wrap(x) for x in v)
        return v

    def __setitem__(self, k, v):
        super(AttrDict, self).__setitem__(k, AttrDict._wrap(v))

    def __setattr__(self, k, v):
        self[k] = v

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)

    def __delattr__(self, k):
        try:
            del self[k]
        except KeyError:
            raise AttributeError(k)


def options(option_dict):
    """utils/common.py:470-471 (EasyDict there)."""
    return AttrDict(option_dict)


def iou(boxes1, boxes2):
    """utils/common.py:451-468: float64 IoU matrix [n1,n2], +1 pixel convention.  Runs on the GPU
    (vdet_iou_f64); bit-exact with the numpy expression of the reference."""
    from .. import ops
    return ops.iou(boxes1, boxes2)


def rcnn_img_crop(img, in_bbox, crop_mode, crop_size, padding, image_mean=None):
    """utils/common.py:208-266 for one window, on the GPU: img uint8 [H,W,3], in_bbox four 1-based inclusive coordinates ->
    float32 [crop_size,crop_size,3], the warped window minus ``image_mean`` on a zero canvas.  ValueError where the reference
    raises inside cv2.resize (an empty window).  Many boxes of one frame: ``ops.rcnn_patches`` / ``googlenet_features`` upload
    the frame once.  RuntimeError without a GPU (no CPU fallback)."""
    import numpy as np
    import torch
    from .. import _lib, ops
    _lib.get_context()        # no library or no GPU: RuntimeError
    img = np.ascontiguousarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("img must be uint8 [H,W,3]")
    box = np.asarray(in_bbox, dtype=np.float64).reshape(1, 4)
    dev = torch.device('cuda', torch.cuda.current_device())
    out = ops.rcnn_patches(torch.from_numpy(img).to(dev)[None], torch.from_numpy(box).to(dev), crop_size=crop_size, padding=padding,
                           mean=None if image_mean is None else np.asarray(image_mean, dtype=np.float64).reshape(3),
                           mode='square' if crop_mode == 'square' else 'warp')
    if not int(out['ok'][0]):
        raise ValueError("rcnn_img_crop: the window of box %s is empty (the reference raises inside cv2.resize)" % (box[0].tolist(),))
    return out['patches'][0].permute(1, 2, 0).contiguous().cpu().numpy()


def im_transform(image, size=-1, scale=1., mean_values=[0., 0., 0.]):
    """utils/common.py:268-280 for ``size <= 0`` (the only branch RCNNProcesser uses): (image - mean_values) * scale,
    [H,W,3] -> [3,H,W].  The resizing branch (cv2.resize of a uint8 crop, googlenet_det's) is out of scope."""
    import numpy as np
    assert len(mean_values) == 3
    if size > 0:
        raise NotImplementedError("im_transform: only size <= 0 (no resize) is provided; see DESIGN.md section 10j")
    trans_img = (np.asarray(image) - np.asarray(mean_values)) * scale
    return trans_img.swapaxes(1, 2).swapaxes(0, 1)


def pickle(data, file_path):
    with open(file_path, 'wb') as f:
        _pickle.dump(data, f, _pickle.HIGHEST_PROTOCOL)


def unpickle(file_path):
    with open(file_path, 'rb') as f:
        return _pickle.load(f)


def read_list(file_path, coding=None):
    """One stripped string per line (utils/common.py:28-35)."""
    if coding is None:
        with open(file_path, 'r') as f:
            return [line.strip() for line in f.readlines()]
    with codecs.open(file_path, 'r', coding) as f:
        return [line.strip() for line in f.readlines()]


def write_list(arr, file_path, coding=None):
    """utils/common.py:38-45: items joined by newlines, no trailing newline."""
    if coding is None:
        with open(file_path, 'w') as f:
            f.write('\n'.join('{}'.format(item) for item in arr))
    else:
        with codecs.open(file_path, 'w', coding) as f:
            f.write(u'\n'.join(arr))


def _tryint(s):
    try:
        return int(s)
    except ValueError:
        return s


def alphanum_key(s):
    """"z23a" -> ["z", 23, "a"] (utils/common.py:129-133)."""
    return [_tryint(c) for c in re.split('([0-9]+)', s)]


def sort_nicely(l):
    """In-place human sort (utils/common.py:135-138)."""
    l.sort(key=alphanum_key)


def basename(file_path):
    return os.path.basename(file_path)


def stem(file_path):
    return os.path.splitext(os.path.basename(file_path))[0]


def isimg(name):
    return name.lower().endswith(('.jpeg', '.png', '.jpg'))


def imread(image_path):
    """utils/common.py:375-376 reads with OpenCV.  The CNN side is external to this build; callers
    that need pixels inject their own reader (``video_det.imread = ...``)."""
    try:
        import cv2
    except ImportError:
        raise RuntimeError("imread needs OpenCV (the image/CNN side is external to vdetlib_amd); "
                           "assign your own reader to the module attribute `imread`")
    return cv2.imread(image_path, cv2.IMREAD_COLOR)


def temp_file(suffix=''):
    f, name = tempfile.mkstemp(suffix=suffix)
    os.close(f)
    return name


def quick_args(arglist):
    """utils/common.py:406-413: positional args, optionally (name, type) tuples."""
    parser = argparse.ArgumentParser()
    for arg in arglist:
        if type(arg) == tuple:
            parser.add_argument(arg[0], type=arg[1])
        else:
            parser.add_argument(arg)
    return parser.parse_args()


def svm_from_rcnn_model(rcnn_model):
    """utils/common.py:416-423: the SVM head of an R-CNN .mat model -- ``W`` [K,M] and ``B`` [1,M] of
    ``rcnn_model.detectors`` and the scalar ``training_opts.feat_norm_mean`` -- as ``image_det.svm_scores`` and
    ``ops.svm_head`` read it."""
    import scipy.io as sio
    rcnn_model = sio.loadmat(rcnn_model)['rcnn_model']
    detectors = rcnn_model['detectors'][0, 0]
    svm = {}
    svm['W'] = detectors['W'][0, 0]
    svm['B'] = detectors['B'][0, 0]
    svm['feat_norm_mean'] = rcnn_model['training_opts'][0, 0]['feat_norm_mean'][0, 0][0, 0]
    return svm
