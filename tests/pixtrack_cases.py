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


# ---------------------------------------------------------------------------------------------------------------------
# the mixed [3,5] slot table: one video per (grid, radius), every kind of slot in one call
# ---------------------------------------------------------------------------------------------------------------------
# LEAVER.  A step can only take a box out of the image when nothing of the winning window is inside it, so a moving object is
# never followed out: its last visible sliver decides.  The case that ends a chain "wholly outside" is built on the edge
# replication instead.  The strip is vertical stripes (every row the same) on frames 0 .. LEAVES-1; from frame LEAVES on only
# row 0 keeps the stripes, the rows below are noise.  The box is S/2 wide and 2S high (a cell is two rows) with its bottom row
# on image row 2R - 1, most of it above the image.  On the striped frames every dy ties and the box stays.  On frame LEAVES
# the window of dy = -R ends on row -1: all of it is the replicated row 0, SAD 0; dy = -R + 1 ends on row 1, which is noise.
LEAVES = 3


def strip_width(S, R):
    return S // 2 + R + 4


def leaver_strip(rng, F, H, S, R):
    """the LEAVER's strip, uint8 [F,H,strip_width,3] drawn from ``rng``: the image's rightmost columns"""
    sw = strip_width(S, R)
    strip = rng.randint(0, 256, size=(F, H, sw, 3)).astype(np.uint8)
    stripes = rng.randint(0, 256, size=(sw, 3)).astype(np.uint8)
    strip[:LEAVES] = stripes
    strip[LEAVES:, 0] = stripes
    return strip


def leaver_box(W, S, R):
    """the LEAVER's anchor box (1-based) on an image W wide that ends in leaver_strip; anchored on frame 1 it goes forward only"""
    x3 = W - strip_width(S, R) + R // 2 + 2
    return [x3 + 1, 2 * R - 2 * S + 1, x3 + S // 2, 2 * R]


FM, HM, WM = 12, 96, 128
PLANT = {8: (16, 8), 32: (64, 64), 64: (64, 64), 12: (24, 36)}     # the planted mover's w, h: whole multiples of the grid
_mixed = {}


def mixed_case(S, R):
    """12 frames of 96 x 128 noise with (1) a planted mover (planted_video), (2) a 37 x 53 white-noise object that moves
    (3, 2) pixels a frame -- the pitch is no integer, the spec itself drifts --, (3) on the right a strip for the box that
    leaves the image (see LEAVER).  -> (images, anchor_frames [3,5], anchor_boxes [3,5,4], anchor_scores [3,5], the mover's
    positions [F,2], its (w, h)); computed once per (S, R) and shared (do not modify)"""
    if (S, R) not in _mixed:
        w, h = PLANT[S]
        anchor = 6
        images, pos = planted_video(3000 + S, FM, HM, WM - strip_width(S, R), w, h, S, R, anchor)
        rng = np.random.RandomState(3100 + S)
        tex2 = rng.randint(0, 256, size=(53, 37, 3)).astype(np.uint8)
        for f in range(FM):
            x2, y2 = 5 + 3 * f, 10 + 2 * f
            images[f, y2:y2 + 53, x2:x2 + 37] = tex2
            images[f, pos[f, 1]:pos[f, 1] + h, pos[f, 0]:pos[f, 0] + w] = planted_texture(3000 + S, w, h)   # the mover on top
        images = np.concatenate([images, leaver_strip(rng, FM, HM, S, R)], axis=2)
        px1, py1 = pos[anchor]
        pxl, pyl = pos[FM - 1]
        mover = [px1 + 1, py1 + 1, px1 + w, py1 + h]
        fr = np.array([[0, anchor + 1, 4, 2, 0],
                       [3, 5, 7, 9, 11],
                       [1, FM, anchor + 1, 0, 0]], np.int32)
        bx = np.zeros((3, 5, 4), np.float32)
        bx[0, 1] = mover
        bx[0, 2] = [5 + 9 + 1, 10 + 6 + 1, 5 + 9 + 37, 10 + 6 + 53]           # the 37 x 53 object on frame 4 (index 3)
        bx[0, 3] = [60, 40, 64, 46]                                           # 5 x 7: w < S
        bx[0, 4] = [7, 7, 9, 9]                                               # (an empty slot's box is not looked at)
        bx[1, 0] = [-20.5, 30, 25, 70]                                        # over the left edge
        bx[1, 1] = [40, -15, 80, 20]                                          # the top
        bx[1, 2] = [110, 20, 150.75, 60]                                      # the right
        bx[1, 3] = [30, 80, 70, 120]                                          # the bottom
        bx[1, 4] = [-30, -25, 10.5, 12.25]                                    # negative coordinates
        bx[2, 0] = leaver_box(WM, S, R)                                       # the leaver, anchored on frame 1: forward only
        bx[2, 1] = [pxl + 1, pyl + 1, pxl + w, pyl + h]                       # the mover anchored on frame F: backward only
        bx[2, 2] = np.array(mover, np.float32) + np.float32([0.75, 0.5, 0.25, 0.99])     # fractional: truncated to the mover
        sc = rng.rand(3, 5).astype(np.float32)
        _mixed[(S, R)] = (images, fr, bx, sc, pos, (w, h))
    return _mixed[(S, R)]
