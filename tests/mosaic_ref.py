"""The picture contract of yv7_mosaic (include/yv7.h, steps a-f) restated in numpy, for the tests.

It paints step after step and tile after tile in painter's order with clipped slice assignments: the canvas, the
tiles (oracle.letterbox_ref.resize_linear_u8), the rows (tests/draw_ref.py's draw_one), the captions' cells, the
borders' bands, and then the box filter as two exact integer matrix products.  It shares no logic with the kernels,
which decide every pixel on their own."""
import math

import numpy as np

import draw_ref as R
from oracle.letterbox_ref import resize_linear_u8

F = np.float32
THICKNESS = 3
CAPTION = 220


def to_u8(images):
    """[B, 3, H, W] uint8 as is; fp16 / fp32 in [0, 1] -> clamp(trunc(float32(x) * 255), 0, 255), NaN -> 0."""
    images = np.asarray(images)
    if images.dtype == np.uint8:
        return images
    with np.errstate(invalid='ignore', over='ignore'):
        f = images.astype(np.float32) * F(255.0)
        f = np.where(np.isnan(f), F(0.0), f)
        return np.trunc(np.clip(f, F(0.0), F(255.0))).astype(np.uint8)


def conf_digit(conf):
    """n with '%.1f' % conf == f'{n // 10}.{n % 10}' for an fp32 conf in [0, 1]."""
    return int(min(max(np.rint(np.float64(F(conf)) * 10.0), 0.0), 10.0))


def pred_label(name, conf):
    n = conf_digit(conf)
    return bytes(name) + b' ' + f'{n // 10}.{n % 10}'.encode()


def block(i, ns, tile_h, tile_w):
    return tile_w * (i // ns), tile_h * (i % ns)


def _draw_row(img, row, label_of, palette, names, atlas):
    row = [float(v) for v in row]
    if not all(math.isfinite(v) for v in row) or row[5] < 0:
        return
    cls = int(row[5])
    label = label_of(names[cls], row[4]) if names is not None and cls < len(names) else None
    R.draw_one(img, row, palette[cls % len(palette)], THICKNESS, label, atlas)


def pred_rows(det, count, n, ns, tile_h, tile_w, sf):
    """The rows step c draws for predictions, in order, in mosaic coordinates: float32 [k, 6]."""
    det = np.asarray(det, np.float32)
    rows = []
    with np.errstate(invalid='ignore', over='ignore'):
        for i in range(n):
            bx, by = block(i, ns, tile_h, tile_w)
            for r in range(min(max(int(count[i]), 0), det.shape[1])):
                row = det[i, r].copy()
                if not row[4] > F(0.25):
                    continue
                if sf < 1:
                    row[:4] = row[:4] * F(sf)
                row[0] += F(bx); row[2] += F(bx); row[1] += F(by); row[3] += F(by)
                rows.append(row)
    return np.array(rows, np.float32).reshape(-1, 6)


def label_rows(targets, label_off, n, ns, tile_h, tile_w, sf, normalized):
    """The rows step c draws for labels: (x1, y1, x2, y2, 1, class) float32 [k, 6]."""
    targets = np.asarray(targets, np.float32).reshape(-1, 6)
    L = len(targets)
    rows, taken = [], set()
    with np.errstate(invalid='ignore', over='ignore'):
        for i in range(n):
            bx, by = block(i, ns, tile_h, tile_w)
            lo, hi = (min(max(int(label_off[k]), 0), L) for k in (i, i + 1))
            for j in range(lo, hi):
                if j in taken:
                    continue
                taken.add(j)
                _, cls, x, y, w, h = targets[j]
                hw, hh = w / F(2), h / F(2)
                c = np.array([x - hw, y - hh, x + hw, y + hh], np.float32)
                if normalized:
                    c = c * np.array([tile_w, tile_h, tile_w, tile_h], np.float32)
                elif sf < 1:
                    c = c * F(sf)
                c = c + np.array([bx, by, bx, by], np.float32)
                rows.append([*c, F(1.0), cls])
    return np.array(rows, np.float32).reshape(-1, 6)


def paint_caption(img, text, bx, by, atlas):
    metrics, cover = atlas
    th = cover.shape[0]
    h, w = img.shape[:2]
    x, top = bx + 5, by + 5
    for b in text:
        g = (b - 32) if 32 <= b <= 126 else ord('?') - 32
        col, adv = int(metrics[g, 0]), int(metrics[g, 1])
        x0, y0, x1, y1 = max(x, 0), max(top, 0), min(x + adv, w), min(top + th, h)
        if x0 < x1 and y0 < y1:
            a = cover[y0 - top:y1 - top, col + x0 - x:col + x1 - x].astype(np.int64)[:, :, None]
            img[y0:y1, x0:x1] = (a * CAPTION + (255 - a) * img[y0:y1, x0:x1].astype(np.int64) + 127) // 255
        x += adv


def paint_border(img, bx, by, tile_h, tile_w):
    X0, Y0, X1, Y1 = bx, by, bx + tile_w, by + tile_h
    white = (255, 255, 255)
    for X in (X0, X1):
        R._fill(img, X - 1, Y0 - 1, X + 1, Y1 + 1, white)
    for Y in (Y0, Y1):
        R._fill(img, X0 - 1, Y - 1, X1 + 1, Y + 1, white)


def area_weights(src, dst):
    """int64 [dst, src]: w(X, x) = max(0, min((X + 1) * src, (x + 1) * dst) - max(X * src, x * dst))."""
    X = np.arange(dst, dtype=np.int64)[:, None]
    x = np.arange(src, dtype=np.int64)[None, :]
    return np.maximum(0, np.minimum((X + 1) * src, (x + 1) * dst) - np.maximum(X * src, x * dst))


def area_resize(img, out_h, out_w):
    Hs, Ws = img.shape[:2]
    if (out_h, out_w) == (Hs, Ws):
        return img.copy()
    wy, wx = area_weights(Hs, out_h), area_weights(Ws, out_w)
    area = Hs * Ws
    assert 255 * area < 2 ** 53     # so the float64 products and sums of these integers are exact (and use BLAS)
    wy, wx = wy.astype(np.float64), wx.T.astype(np.float64)
    out = np.empty((out_h, out_w, 3), np.uint8)
    for c in range(3):
        out[:, :, c] = ((wy @ img[:, :, c].astype(np.float64) @ wx).astype(np.int64) + area // 2) // area
    return out


def mosaic(images, n, ns, tile_h, tile_w, sf, out_h, out_w, det=None, count=None, targets=None, label_off=None,
           normalized=True, palette=None, names=None, atlas=None, captions=None, full=False):
    """The output picture uint8 [out_h, out_w, 3] (full: the mosaic before step f).  images [B, 3, H, W];
    captions: one bytes per tile, or None; names: a list of bytes, or None."""
    u8 = to_u8(images)
    H, W = u8.shape[2:]
    img = np.full((ns * tile_h, ns * tile_w, 3), 255, np.uint8)                       # a
    for i in range(n):                                                                # b
        bx, by = block(i, ns, tile_h, tile_w)
        tile = np.ascontiguousarray(u8[i].transpose(1, 2, 0))
        if (tile_h, tile_w) != (H, W):
            tile = resize_linear_u8(tile, tile_w, tile_h)
        img[by:by + tile_h, bx:bx + tile_w] = tile
    if det is not None:                                                               # c
        for row in pred_rows(det, count, n, ns, tile_h, tile_w, sf):
            _draw_row(img, row, pred_label, palette, names, atlas)
    elif label_off is not None:
        for row in label_rows(targets, label_off, n, ns, tile_h, tile_w, sf, normalized):
            _draw_row(img, row, lambda name, conf: bytes(name), palette, names, atlas)
    if captions is not None:                                                          # d
        for i in range(n):
            paint_caption(img, captions[i], *block(i, ns, tile_h, tile_w), atlas)
    for i in range(n):                                                                # e
        paint_border(img, *block(i, ns, tile_h, tile_w), tile_h, tile_w)
    return img if full else area_resize(img, out_h, out_w)                            # f
