"""A gfx950 temporal-convolution network with pycaffe's calling convention, to plug into
``score_conv_cls`` (reference vdet/tubelet_cls.py:15-51).

The reference feeds per-tubelet channel sequences to an external Caffe TCN whose prototxt/weights
are NOT part of the reference tree, so the architecture here is the build's own (parity unpinned,
DESIGN.md section 2): a stack of 1-D "same" convolutions over the tubelet length, ReLU between
layers, a 2-way softmax at the end; ``forward()`` returns ``{'probs': [1, 2, L]}`` like the
reference expects (:47-48).  Every layer runs on the GPU (vdet_conv1d_f32).
"""
import ctypes

import numpy as np

from .. import _lib


class Blob(object):
    """Minimal pycaffe blob: .shape, .reshape(*dims), .data (numpy float32)."""

    def __init__(self, channels):
        self.shape = (1, channels, 1, 1)
        self.data = np.zeros(self.shape, dtype=np.float32)

    def reshape(self, *dims):
        self.shape = tuple(int(d) for d in dims)
        self.data = np.zeros(self.shape, dtype=np.float32)


class TCNNet(object):
    """inputs: ordered list of (blob_name, channels) concatenated along the channel axis;
    layers: list of (W [Cout,Cin,K] float32, b [Cout] float32); the last layer must have Cout == 2."""

    def __init__(self, inputs, layers):
        self.inputs = [(n, int(c)) for n, c in inputs]
        self.blobs = {n: Blob(c) for n, c in self.inputs}
        self.layers = [(np.ascontiguousarray(w, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32))
                       for w, b in layers]
        cin = sum(c for _, c in self.inputs)
        for w, b in self.layers:
            if w.ndim != 3 or w.shape[1] != cin or w.shape[2] % 2 != 1 or b.shape != (w.shape[0],):
                raise ValueError("layer shapes do not chain: %r after %d channels" % (w.shape, cin))
            cin = w.shape[0]
        if cin != 2:
            raise ValueError("the last layer must produce 2 channels (probs[:, 1, :] is the score)")

    @staticmethod
    def random(inputs, hidden=(16, 16), kernel=3, seed=0):
        rng = np.random.RandomState(seed)
        cin = sum(c for _, c in inputs)
        layers = []
        for cout in list(hidden) + [2]:
            layers.append((rng.randn(cout, cin, kernel).astype(np.float32) / np.sqrt(cin * kernel),
                           (0.1 * rng.randn(cout)).astype(np.float32)))
            cin = cout
        return TCNNet(inputs, layers)

    @staticmethod
    def from_npz(inputs, path):
        """Weights saved as ``w0, b0, w1, b1, ...`` (e.g. by vdetlib_amd.tools.caffemodel_to_npz)."""
        z = np.load(path)
        layers = []
        i = 0
        while 'w%d' % i in z.files:
            layers.append((z['w%d' % i], z['b%d' % i]))
            i += 1
        return TCNNet(inputs, layers)

    def save_npz(self, path):
        arrs = {}
        for i, (w, b) in enumerate(self.layers):
            arrs['w%d' % i] = w
            arrs['b%d' % i] = b
        np.savez(path, **arrs)

    # channel codes of include/vdet_hip.h (vdet_tcn_tracks): the blob names the device assembly knows
    DEVICE_CHANNELS = {'det_scores': 0, 'track_scores': 1, 'anchors': 2, 'abs_anchors': 3, 'gt_overlaps': 4, 'labels': 5}

    def packed(self):
        """(params f32 = W0 | b0 | W1 | b1 ..., layers int32 [n,3] = (Cout, Cin, K)): the form the one-launch entry points
        take (vdet_tcn_tracks, vdet_tcn_series_f32).  Built once and kept, so that the library finds the same bytes at
        the same address on every call; a net whose ``layers`` were edited in place needs a fresh TCNNet."""
        if getattr(self, '_packed', None) is None:
            params = np.concatenate([a.ravel() for w, b in self.layers for a in (w, b)]).astype(np.float32)
            shapes = np.array([w.shape for w, _ in self.layers], dtype=np.int32).reshape(-1, 3)
            self._packed = (np.ascontiguousarray(params), np.ascontiguousarray(shapes))
        return self._packed

    def device_channels(self):
        """The input list as channel codes of the device assembly; ValueError for blobs it cannot assemble
        (``all_scores`` / ``feats``, multi-channel blobs, unknown names: those travel as rows, ``device_inputs``)."""
        codes = []
        for name, ch in self.inputs:
            if name not in self.DEVICE_CHANNELS or ch != 1:
                raise ValueError("the device TCN assembles one-channel blobs named %s; got %r with %d channel(s)"
                                 % (sorted(self.DEVICE_CHANNELS), name, ch))
            codes.append(self.DEVICE_CHANNELS[name])
        return np.array(codes, dtype=np.int32)

    def device_inputs(self, wide):
        """The input list for the wide entry points (vdet_tcn_tracks_wide): per input ``(code, channels)``, code -1 for
        a blob whose name is in ``wide`` (per-box rows, e.g. ``all_scores`` / ``feats``), else its ``DEVICE_CHANNELS``
        code.  ValueError: a device-channel name in ``wide``, a one-channel name with more than one channel, a blob
        that is neither, more than 16 inputs, more than 4096 channels together."""
        clash = sorted(set(wide) & set(self.DEVICE_CHANNELS))
        if clash:
            raise ValueError("%r is assembled on the device and cannot be a wide blob" % clash)
        unused = sorted(set(wide) - set(n for n, _ in self.inputs))
        if unused:
            raise ValueError("the net has no blob named %r" % unused)
        if len(self.inputs) > 16:
            raise ValueError("the device TCN takes at most 16 inputs; the net has %d" % len(self.inputs))
        out = []
        for name, ch in self.inputs:
            if name in wide:
                if not 1 <= ch <= 4096:
                    raise ValueError("a wide blob has 1 to 4096 channels; %r has %d" % (name, ch))
                out.append((-1, ch))
            elif name in self.DEVICE_CHANNELS and ch == 1:
                out.append((self.DEVICE_CHANNELS[name], 1))
            else:
                raise ValueError("the device TCN assembles one-channel blobs named %s and reads wide blobs from the rows "
                                 "passed as wide={name: rows}; got %r with %d channel(s) and no rows"
                                 % (sorted(self.DEVICE_CHANNELS), name, ch))
        if sum(ch for _, ch in out) > 4096:
            raise ValueError("the device TCN takes at most 4096 input channels")
        return out

    def forward_series(self, series, ctx=None):
        """The net on many series in ONE launch (vdet_tcn_series_f32): ``series`` is a list of float32 arrays
        [Cin, L_t] (the channels in ``inputs`` order); returns the list of probs[1] arrays [L_t] -- what ``forward()``
        gives as ``['probs'][0, 1]`` series by series, bit for bit."""
        cin = sum(c for _, c in self.inputs)
        xs = []
        for x in series:
            x = np.ascontiguousarray(x, dtype=np.float32)
            if x.ndim != 2 or x.shape[0] != cin:
                raise ValueError("every series must be [%d, L]; got %r" % (cin, x.shape))
            xs.append(x)
        lens = np.array([x.shape[1] for x in xs], dtype=np.int64)
        off = np.zeros(len(xs) + 1, dtype=np.int64)
        np.cumsum(lens, out=off[1:])
        flat = np.concatenate([x.ravel() for x in xs]) if xs else np.zeros(0, np.float32)
        flat = np.ascontiguousarray(flat, dtype=np.float32)
        out = np.empty(int(off[-1]), dtype=np.float32)
        params, shapes = self.packed()
        if ctx is None:
            ctx = _lib.get_context()
            ctx.reset_stream()
        ctx.check(ctx.lib.vdet_tcn_series_f32(ctx.h, params.ctypes.data, shapes.ctypes.data, len(self.layers), cin,
                                              flat.ctypes.data, off.ctypes.data, len(xs), out.ctypes.data))
        return [out[off[i]:off[i + 1]] for i in range(len(xs))]

    def forward(self):
        L = self.blobs[self.inputs[0][0]].shape[3]
        x = np.concatenate([np.asarray(self.blobs[n].data, dtype=np.float32).reshape(c, L) for n, c in self.inputs], 0)
        x = np.ascontiguousarray(x)
        ctx = _lib.get_context()
        ctx.reset_stream()
        for li, (w, b) in enumerate(self.layers):
            act = 2 if li == len(self.layers) - 1 else 1
            out = np.empty((w.shape[0], L), dtype=np.float32)
            ctx.check(ctx.lib.vdet_conv1d_f32(ctx.h, x.ctypes.data, x.shape[0], L, w.ctypes.data, b.ctypes.data,
                                              w.shape[0], w.shape[2], act, out.ctypes.data))
            x = out
        return {'probs': x[None]}
