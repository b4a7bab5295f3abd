"""The wide first layer of the device TCN (csrc/tcn_kernels.hpp, tcn_wide_layer_kernel) stated in numpy f32: how a net's
inputs concatenate into [Cin, L] and the order in which layer 0 sums.  Every product and every sum is an explicit
``np.float32`` operation, so the statement rounds where the kernel rounds and nowhere else.  Shared by
tests/test_tcn_wide_cpu.py and tests/test_tcn_wide_gpu.py; it is not the code under test."""
import numpy as np

f32 = np.float32


def widen_rows(rows):
    """Rows as the kernel reads them: f32 as it is, f16 exactly, f64 rounded once to nearest (np.asarray(.., 'float32'))."""
    return np.asarray(rows).astype(np.float32)


def concat_inputs(inputs, series, wide, frames):
    """x [Cin, L] f32 of one tubelet.  ``inputs``: the net's (name, channels) list; ``series``: name -> [L] values of the
    one-channel inputs (already compacted); ``wide``: name -> rows [F, W] of this tubelet slot; ``frames``: the 0-based frames
    of its boxes in order.  Channel q of a wide blob at series position j is entry q of the row of the j-th box."""
    frames = np.asarray(frames, dtype=np.int64)
    parts = []
    for name, ch in inputs:
        if name in wide:
            rows = widen_rows(wide[name])
            assert rows.ndim == 2 and rows.shape[1] == ch, (name, rows.shape, ch)
            parts.append(np.ascontiguousarray(rows[frames].T))
        else:
            assert ch == 1
            parts.append(np.asarray(series[name], dtype=np.float32).reshape(1, len(frames)))
    return np.concatenate(parts, 0)


def layer0(x, w, b, relu):
    """[Cout, L] f32: acc = b[co]; ci ascending, k inner; p = w * x rounded to f32, acc = acc + p.  A position outside the
    series enters as +0.0f and its product IS added.  ReLU as the kernels write it: ``acc > 0 ? acc : 0``."""
    x = np.asarray(x, dtype=np.float32)
    w = np.asarray(w, dtype=np.float32)
    cout, cin, K = w.shape
    assert x.shape[0] == cin and K % 2 == 1
    L = x.shape[1]
    h = K // 2
    xp = np.zeros((cin, L + 2 * h), np.float32)
    xp[:, h:h + L] = x
    with np.errstate(all='ignore'):
        acc = np.repeat(np.asarray(b, dtype=np.float32)[:, None], L, axis=1)      # [Cout, L]: every (co, position) its own chain
        for ci in range(cin):
            for k in range(K):
                p = w[:, ci, k][:, None] * xp[ci, k:k + L][None, :]               # f32 * f32 -> f32: one rounding
                acc = acc + p                                                     # f32 + f32 -> f32: one rounding
        assert acc.dtype == np.float32 and p.dtype == np.float32
        return np.where(acc > 0, acc, f32(0)) if relu else acc


def layer0_f64(x, w, b):
    """(value, bound) in f64: the exact-ish sum and |b| + sum |w * x| per output, for the recursive-summation bound."""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    cout, cin, K = w.shape
    L = x.shape[1]
    h = K // 2
    xp = np.zeros((cin, L + 2 * h))
    xp[:, h:h + L] = x
    val = np.tile(np.asarray(b, dtype=np.float64)[:, None], (1, L))
    mag = np.abs(val)
    for k in range(K):
        val += w[:, :, k] @ xp[:, k:k + L]
        mag += np.abs(w[:, :, k]) @ np.abs(xp[:, k:k + L])
    return val, mag
