"""Seeded videos for the pixel tracker's tests (CPU: the spec against known positions; GPU: the device against the spec)."""
import numpy as np


def planted_video(seed, F, H, W, w, h, S, R, anchor, vanish_from=None):
    """A seeded uint8 texture (3 channels) of w x h pixels pasted over fresh seeded noise on every frame.  Its per-frame moves
    are whole multiples of the grid pitch (w // S, h // S pixels), at most R - 1 cells, and keep it inside the image.  From
    frame ``vanish_from`` (0-based) on the frames are noise only.  Returns (images [F,H,W,3], positions [F,2] of the 0-based
    (x1, y1); the walk starts anywhere, ``anchor`` is only the frame the caller will anchor on)."""
    assert w % S == 0 and h % S == 0 and w <= W and h <= H
    rng = np.random.RandomState(seed)
    tex = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    px, py = w // S, h // S
    x, y = ((W - w) // (2 * px)) * px, ((H - h) // (2 * py)) * py
    pos = np.zeros((F, 2), np.int64)
    images = rng.randint(0, 256, size=(F, H, W, 3)).astype(np.uint8)
    for f in range(F):
        if f:
            mx, my = (int(v) for v in rng.randint(-(R - 1), R, size=2))
            if not 0 <= x + mx * px <= W - w:
                mx = -mx
            if not 0 <= x + mx * px <= W - w:
                mx = 0
            if not 0 <= y + my * py <= H - h:
                my = -my
            if not 0 <= y + my * py <= H - h:
                my = 0
            x, y = x + mx * px, y + my * py
        pos[f] = (x, y)
        if vanish_from is None or f < vanish_from:
            images[f, y:y + h, x:x + w] = tex
    return images, pos


def planted_texture(seed, w, h):
    """the texture planted_video(seed, ...) pastes (its first draw)"""
    return np.random.RandomState(seed).randint(0, 256, size=(h, w, 3)).astype(np.uint8)


def rows_from_positions(pos, w, h, frames):
    """[F,5] f32 rows (1-based box, 1.0) on ``frames``, NaN elsewhere"""
    rows = np.full((len(pos), 5), np.nan, np.float32)
    for f in frames:
        x, y = pos[f]
        rows[f] = (x + 1, y + 1, x + w, y + h, 1.0)
    return rows
