"""The drawing contract of yv7_draw_boxes (include/yv7.h) restated in numpy, for the tests.

It paints one primitive after the other in painter's order with clipped slice assignments — outline (four bands),
label background, then the glyph cells one by one — so it shares no logic with the kernel, which decides
every pixel on its own by searching for the last primitive that covers it."""
import math

import numpy as np

TEXT = (225, 255, 255)


def conf_digits(conf):
    """n with f'{conf:.2f}' == f'{n // 100}.{n % 100:02d}' for an fp32 conf in [0, 1]: an fp32 times 100 is exact
    in double, and rint is round half to even."""
    return int(min(max(np.rint(np.float64(np.float32(conf)) * 100.0), 0.0), 100.0))


def label_text(name, conf):
    n = conf_digits(conf)
    return bytes(name) + b' ' + f'{n // 100}.{n // 10 % 10}{n % 10}'.encode()


def _fill(img, x0, y0, x1, y1, colour):
    """colour on x0..x1, y0..y1 inclusive, clipped."""
    h, w = img.shape[:2]
    x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, w - 1), min(y1, h - 1)
    if x0 <= x1 and y0 <= y1:
        img[y0:y1 + 1, x0:x1 + 1] = colour


def draw_one(img, row, colour, t, label=None, atlas=None):
    """One det row (x1, y1, x2, y2, conf, cls) onto img (uint8 HWC, in place).  label: the text's bytes or None;
    atlas: (metrics int [95, 2] of (column, advance), cover uint8 [cell_h, total_w])."""
    x1, y1, x2, y2 = (int(v) for v in row[:4])     # truncation toward zero
    xa, xb, ya, yb = min(x1, x2), max(x1, x2), min(y1, y2), max(y1, y2)
    lo = t // 2
    X0, X1, Y0, Y1 = xa - lo, xb - lo + t - 1, ya - lo, yb - lo + t - 1
    _fill(img, X0, Y0, X1, ya - lo + t - 1, colour)        # top band
    _fill(img, X0, yb - lo, X1, Y1, colour)                # bottom band
    _fill(img, X0, Y0, xa - lo + t - 1, Y1, colour)        # left band
    _fill(img, xb - lo, Y0, X1, Y1, colour)                # right band
    if label is None:
        return
    metrics, cover = atlas
    th = cover.shape[0]
    glyphs = [(b - 32) if 32 <= b <= 126 else ord('?') - 32 for b in label]
    tw = sum(int(metrics[g, 1]) for g in glyphs)
    _fill(img, xa, ya - th - 3, xa + tw, ya, colour)
    h, w = img.shape[:2]
    x, top = xa, ya - 1 - th
    text, base = np.array(TEXT, np.int64), np.array([int(c) for c in colour], np.int64)
    for g in glyphs:                                       # one clipped cell after the other
        col, adv = int(metrics[g, 0]), int(metrics[g, 1])
        x0, y0, x1, y1 = max(x, 0), max(top, 0), min(x + adv, w), min(top + th, h)
        if x0 < x1 and y0 < y1:
            a = cover[y0 - top:y1 - top, col + x0 - x:col + x1 - x].astype(np.int64)[:, :, None]
            img[y0:y1, x0:x1] = (a * text + (255 - a) * base + 127) // 255
        x += adv


def draw(img, det, palette, t, names=None, atlas=None, reverse=False):
    """A copy of img with det's rows [n, 6] drawn in order (reverse: last row first).  names: a list of bytes."""
    out = np.array(img, dtype=np.uint8, copy=True)
    rows = [[float(v) for v in r] for r in np.asarray(det, dtype=np.float32).reshape(-1, 6)]
    for r in (rows[::-1] if reverse else rows):
        if not all(math.isfinite(v) for v in r) or r[5] < 0:
            continue
        cls = int(r[5])
        label = label_text(names[cls], r[4]) if names is not None and cls < len(names) else None
        draw_one(out, r, palette[cls % len(palette)], t, label, atlas)
    return out


def synthetic_atlas(cell_h=4):
    """Every glyph two columns wide with coverage 255, but three: 'a' 2 wide at 0, 'b' 3 wide at 128, 'c' 5 wide at
    255 in a checkerboard over 0.  Total width 2 * 92 + 2 + 3 + 5."""
    adv = np.full(95, 2, np.int32)
    adv[ord('a') - 32], adv[ord('b') - 32], adv[ord('c') - 32] = 2, 3, 5
    col = np.concatenate([[0], np.cumsum(adv)[:-1]]).astype(np.int32)
    cover = np.full((cell_h, int(adv.sum())), 255, np.uint8)
    cover[:, col[ord('a') - 32]:col[ord('a') - 32] + 2] = 0
    cover[:, col[ord('b') - 32]:col[ord('b') - 32] + 3] = 128
    c0 = col[ord('c') - 32]
    for y in range(cell_h):
        for x in range(5):
            cover[y, c0 + x] = 255 if (x + y) % 2 == 0 else 0
    return np.stack([col, adv], 1).astype(np.int32), cover
