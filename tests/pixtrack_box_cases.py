"""Seeded videos for the box-sampling pixel tracker's tests (CPU: the two specs against the planted track; GPU: the device
against the spec): motion BELOW the grid pitch.  An object of w x h pixels whose texture is white noise in 3 x 3 pixel blocks
is pasted over a background of the same kind and moves by whole pixels, 1 .. 3 on either axis and in either direction, per
frame: never a multiple of the pitch (w / 8 and h / 8 are 4.5 .. 5.5 pixels).  12 frames of 120 x 160, grid 8, radius 3."""
import numpy as np

F, H, W = 12, 120, 160
S, R = 8, 3
BLOCK = 3
SIZES = ((44, 36), (40, 40))           # (w, h) of the object
SEEDS = (0, 1, 2, 3)                   # chosen on the CPU: tests/test_pixel_track_box_cpu.py::test_sub_cell_motion holds on each
KW = dict(grid=S, radius=R, min_conf=0.0)


def _blocky(rng, h, w):
    n = rng.randint(0, 256, size=((h + BLOCK - 1) // BLOCK, (w + BLOCK - 1) // BLOCK)).astype(np.uint8)
    return np.repeat(np.repeat(n, BLOCK, axis=0), BLOCK, axis=1)[:h, :w]


_videos = {}


def sub_cell_video(seed, w, h):
    """-> (images uint8 [F,H,W,3], pos [F,2] int: the planted 0-based (x1, y1) of the object); computed once and shared (do
    not modify)"""
    if (seed, w, h) not in _videos:
        rng = np.random.RandomState(7700 + seed)
        bg, tex = _blocky(rng, H, W), _blocky(rng, h, w)
        x, y = (W - w) // 2, (H - h) // 2
        pos = np.zeros((F, 2), np.int64)
        planes = np.repeat(bg[None], F, axis=0)
        for f in range(F):
            if f:
                mx, my = (int(v) for v in rng.choice([-3, -2, -1, 1, 2, 3], size=2))
                if not 0 <= x + mx <= W - w:
                    mx = -mx
                if not 0 <= y + my <= H - h:
                    my = -my
                x, y = x + mx, y + my
            pos[f] = (x, y)
            planes[f, y:y + h, x:x + w] = tex
        _videos[(seed, w, h)] = (np.repeat(planes[..., None], 3, axis=-1), pos)
    return _videos[(seed, w, h)]


def anchor_of(pos, w, h):
    """([[frame]], [[box]]) of the 1-based anchor on the first frame"""
    x, y = int(pos[0, 0]), int(pos[0, 1])
    return np.array([[1]], np.int32), np.array([[[x + 1, y + 1, x + w, y + h]]], np.float32)


def errors(rows, pos):
    """|x1 - planted|, |y1 - planted| per frame ([F] each; NaN where the chain has no row) of the rows [F,5] (1-based)"""
    return np.abs(rows[:, 0] - 1 - pos[:, 0]), np.abs(rows[:, 1] - 1 - pos[:, 1])
