"""Boxes and labels drawn on the device — the reference's utils/plots.py:29-34, 57-68.

`plot_boxes(frames, det, count, ...)` is plot_one_box for a whole batch: one yv7_draw_boxes call (libyv7, two
launches per 64 images) on nms_batched's fixed-shape output after scale_boxes, stream-ordered, with no host read.
The drawing is defined by the contract in include/yv7.h, not by cv2 (absent here): square corners, no anti-aliased
edges, and the text comes from PIL's default font rendered once into a glyph atlas.  There is no CPU path and no
plot_one_box for one box on a host array.

`plot_images(images, targets, paths, fname, names, ...)` is the reference's picture grid (plots.py:114-190, the
test_batch*_labels.jpg / _pred.jpg of test.py) built on the device by one yv7_mosaic call, and `output_to_target`
its host helper (plots.py:105-111).
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from utils.datasets import _hip_device, pack_frames
from yv7 import _lib as L


def color_list():   # plots.py:29-34: the first ten matplotlib colours as (r, g, b)
    import matplotlib.colors

    def hex2rgb(h):
        return tuple(int(h[1 + i:1 + i + 2], 16) for i in (0, 2, 4))

    return [hex2rgb(h) for h in matplotlib.colors.TABLEAU_COLORS.values()]


def line_thickness(shape):   # plots.py:59: line / font thickness of an image of shape (h, w, ...)
    return round(0.002 * (shape[0] + shape[1]) / 2) + 1


_line_thickness = line_thickness   # plot_boxes has a parameter of that name


def display_channels(C):
    """Which channels of a C-channel frame a 3-channel picture of it shows: the first three, a pair as (0, 1, 1),
    a single band three times.  The drawing and mosaic kernels stay 3-channel and take such copies."""
    return (0, 1, 2) if C >= 3 else (0, 1, 1) if C == 2 else (0, 0, 0)


def display_copy(x, dim):
    """The 3-channel display copy of a device tensor whose channels lie along `dim` ([H, W, C] frames: 2,
    [B, C, H, W] batches: 1), contiguous.  Slices and one cat: nothing here waits for the device."""
    return torch.cat([x.narrow(dim, c, 1) for c in display_channels(x.shape[dim])], dim).contiguous()


def display_frames(frames, device):
    """display_copy of each uint8 [H, W, C] frame (numpy arrays travel in one packed upload, HIP tensors are read in
    place and left as they are) -> a list of [H, W, 3] HIP tensors plot_boxes may draw on."""
    ptrs, keep = pack_frames(frames, device)
    packed = keep[0] if any(isinstance(f, np.ndarray) for f in frames) else None
    out = []
    for f, p in zip(frames, ptrs):
        if isinstance(f, np.ndarray):
            o = p - packed.data_ptr()
            f = packed[o:o + f.size].view(f.shape)
        out.append(display_copy(f, 2))
    return out


def text_height(t):
    """The glyph cell's height for line thickness t.  The reference draws cv2's 22-pixel face at fontScale t / 3;
    22 pixels is that face's height above the baseline, and the cell here also holds the descenders, which in PIL's
    default font of size 22 makes 28 rows.  10 rows (size 8) is the smallest that still reads."""
    return max(round(28 * t / 3), 10)


_ATLAS_HOST, _ATLAS_DEV, _NAMES, _PALETTE = {}, {}, {}, {}


def _font(cell_h):
    """PIL's default font at the largest size whose ascent + descent fits cell_h rows; without FreeType, PIL's
    built-in bitmap font, whatever cell_h."""
    from PIL import ImageFont
    try:
        for size in range(cell_h, 0, -1):
            f = ImageFont.load_default(size)
            if sum(f.getmetrics()) <= cell_h or size == 1:
                return f
    except (OSError, TypeError, AttributeError):
        pass
    return ImageFont.load_default()


def glyph_atlas_host(cell_h):
    """(metrics int32 [95, 2], cover uint8 [cell_h, total_w]) for ASCII 32 .. 126: each glyph's first column and
    advance, and its coverage.  Every glyph is rendered on its own and clipped to its advance."""
    cell_h = int(cell_h)
    if cell_h not in _ATLAS_HOST:
        from PIL import Image, ImageDraw, ImageFont
        font = _font(cell_h)
        scalable = isinstance(font, ImageFont.FreeTypeFont)
        cells = []
        for c in range(32, 127):
            ch = chr(c)
            adv = max(int(math.ceil(font.getlength(ch))), 1)
            rows = cell_h if scalable else max(font.getbbox(ch)[3], 1)
            im = Image.new('L', (adv, rows), 0)
            ImageDraw.Draw(im).text((0, 0), ch, fill=255, font=font)
            cells.append(np.asarray(im, dtype=np.uint8))
        rows = max(c.shape[0] for c in cells)   # the bitmap font: its own height
        cells = [np.pad(c, ((0, rows - c.shape[0]), (0, 0))) for c in cells]
        adv = np.array([c.shape[1] for c in cells], np.int32)
        col = np.concatenate([[0], np.cumsum(adv)[:-1]]).astype(np.int32)
        _ATLAS_HOST[cell_h] = np.stack([col, adv], 1).astype(np.int32), np.ascontiguousarray(np.concatenate(cells, 1))
    return _ATLAS_HOST[cell_h]


class Atlas:
    """A glyph atlas on the device: metrics int32 [95, 2] (column, advance) and cover uint8 [cell_h, total_w]."""

    def __init__(self, metrics, cover, device):
        metrics, cover = np.ascontiguousarray(metrics, np.int32), np.ascontiguousarray(cover, np.uint8)
        if metrics.shape != (95, 2) or cover.ndim != 2:
            raise ValueError(f'glyph atlas: expected metrics [95, 2] and cover [cell_h, total_w], got '
                             f'{metrics.shape} and {cover.shape}')
        if int(metrics[:, 1].sum()) != cover.shape[1]:
            raise ValueError('glyph atlas: the advances must sum to the coverage map\'s width')
        self.cell_h, self.total_w = (int(v) for v in cover.shape)
        self.metrics, self.cover = torch.from_numpy(metrics).to(device), torch.from_numpy(cover).to(device)


def glyph_atlas(cell_h, device=None):
    """The atlas of PIL's default font for a cell of cell_h rows, cached per (cell_h, device)."""
    device = _hip_device(device if device is not None else 'cuda')
    key = int(cell_h), device
    if key not in _ATLAS_DEV:
        _ATLAS_DEV[key] = Atlas(*glyph_atlas_host(int(cell_h)), device)
    return _ATLAS_DEV[key]


def _names_blob(names, device):
    key = tuple(names), device
    if key not in _NAMES:
        raw = [n if isinstance(n, bytes) else str(n).encode('utf-8') for n in names]
        off = np.concatenate([[0], np.cumsum([len(r) for r in raw])]).astype(np.int32)
        blob = np.frombuffer(b''.join(raw) + b'\0', np.uint8).copy()   # never empty
        _NAMES[key] = torch.from_numpy(blob).to(device), torch.from_numpy(off).to(device), len(raw)
    return _NAMES[key]


def _palette(colors, device):
    key = tuple(tuple(int(v) for v in c) for c in colors), device
    if key not in _PALETTE:
        pal = np.array(key[0], np.uint8).reshape(-1, 3)
        _PALETTE[key] = torch.from_numpy(pal).to(device)
    return _PALETTE[key]


def plot_boxes(frames, det, count, names=None, colors=None, line_thickness=None, reverse=False, atlas=None):
    """plot_one_box (plots.py:57-68) for every row < count[b] of every frame, in one yv7_draw_boxes call.

    frames: uint8 HWC numpy arrays (uploaded in one packed copy, left unmodified) or contiguous HIP tensors (drawn
    in place), any sizes.  det [B, max_det, 6] fp32 and count [B] int32 on the device, as nms_batched returns them
    after scale_boxes.  names: class names for 'name conf' labels, None for boxes alone.  colors: (c0, c1, c2)
    tuples in the frames' channel order, default color_list().  line_thickness: one value or one per frame, default
    the reference's rule per frame.  reverse: draw the last row first (detect.py:209).  atlas: an Atlas to use for
    every frame instead of glyph_atlas(text_height(t)).
    Returns the annotated frames as a list of HIP tensors, stream-ordered: nothing is read back."""
    if not (isinstance(det, torch.Tensor) and det.is_cuda):
        raise RuntimeError('plot_boxes draws on a ROCm device (libyv7); got CPU detections')
    device = det.device
    B = len(frames)
    if det.dtype != torch.float32 or det.dim() != 3 or det.shape[0] != B or det.shape[2] != 6 or \
            not det.is_contiguous() or B == 0:
        raise ValueError(f'plot_boxes: expected contiguous fp32 det [B, max_det, 6] for {B} frames')
    if count.dtype != torch.int32 or tuple(count.shape) != (B,) or not count.is_contiguous() or count.device != device:
        raise ValueError('plot_boxes: count must be int32 [B] on det\'s device')
    for f in frames:
        is_t = isinstance(f, torch.Tensor)
        if f.dtype != (torch.uint8 if is_t else np.uint8) or f.ndim != 3 or f.shape[2] != 3:
            raise ValueError(f'plot_boxes: expected uint8 [H, W, 3] frames, got {f.dtype} {tuple(f.shape)}')
        if is_t and not f.is_contiguous():
            raise ValueError('plot_boxes: a tensor frame is drawn in place and must be contiguous')
    max_det = det.shape[1]
    ptrs, keep = pack_frames(frames, device)
    out, packed = [], keep[0] if any(isinstance(f, np.ndarray) for f in frames) else None
    for f, p in zip(frames, ptrs):
        if isinstance(f, torch.Tensor):
            out.append(f)
        else:
            o = p - packed.data_ptr()
            out.append(packed[o:o + f.size].view(f.shape))
    if line_thickness is None:
        ts = [_line_thickness(f.shape) for f in frames]
    else:
        ts = list(line_thickness) if isinstance(line_thickness, (list, tuple)) else [line_thickness] * B
    ts = [int(t) for t in ts]
    if len(ts) != B or min(ts) < 1:
        raise ValueError('plot_boxes: line_thickness must be at least 1, one value or one per frame')

    pal = _palette(colors if colors is not None else color_list(), device)
    atlases, which = [], [0] * B
    if names is not None:
        if atlas is not None:
            atlases = [atlas]
        else:
            heights = sorted({text_height(t) for t in ts})
            if len(heights) > L.DRAW_MAX_ATLAS:
                raise ValueError(f'plot_boxes: more than {L.DRAW_MAX_ATLAS} text heights in one batch')
            atlases = [glyph_atlas(h, device) for h in heights]
            which = [heights.index(text_height(t)) for t in ts]
        blob, off, nc = _names_blob(names, device)
    images = (L.DrawImage * B)()
    for d, p, f, t, a in zip(images, ptrs, frames, ts, which):
        d.data, d.h, d.w, d.thickness, d.atlas = p, f.shape[0], f.shape[1], t, a
    arr = (L.GlyphAtlas * max(len(atlases), 1))()
    for d, a in zip(arr, atlases):
        d.metrics, d.cover, d.cell_h, d.total_w = a.metrics.data_ptr(), a.cover.data_ptr(), a.cell_h, a.total_w
    lib = L.lib()
    ws = torch.empty(int(lib.yv7_draw_ws_bytes(B, max_det)), dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream(device).cuda_stream
        rc = lib.yv7_draw_boxes(images, B, det.data_ptr(), count.data_ptr(), max_det, pal.data_ptr(), pal.shape[0],
                                blob.data_ptr() if names is not None else None,
                                off.data_ptr() if names is not None else None, nc if names is not None else 0,
                                arr if atlases else None, len(atlases), int(bool(reverse)), ws.data_ptr(),
                                ws.numel(), stream)
    L.check(rc, 'yv7_draw_boxes')
    return out


def mosaic_geometry(bs, h, w, max_size=640, max_subplots=16, max_out=1280):
    """The picture grid's sizes with plot_images' own float expressions (plots.py:128-145, 186-187).  max_out is the
    reference's constant 1280.  Returns a dict: n tiles on an ns x ns grid, tile (h, w), sf, mosaic (h, w),
    out (h, w) and blocks [(block_x, block_y)] per tile (tiles fill column by column)."""
    n = min(int(bs), int(max_subplots))
    ns = np.ceil(n ** 0.5)
    sf = max_size / max(h, w)
    if sf < 1:
        h = math.ceil(sf * h)
        w = math.ceil(sf * w)
    r = min(float(max_out) / max(h, w) / ns, 1.0)
    return dict(n=n, ns=int(ns), sf=float(sf), tile=(h, w), mosaic=(int(ns * h), int(ns * w)),
                out=(int(ns * h * r), int(ns * w * r)),
                blocks=[(int(w * (i // ns)), int(h * (i % ns))) for i in range(n)])


def output_to_target(output):
    """plots.py:105-111: NMS output -> [n, 7] numpy rows (batch_id, class_id, x, y, w, h, conf).  output: a list of
    per-image [k, 6] tensors, or nms_batched's (det, count) pair.  A host function (it reads the device)."""
    if isinstance(output, tuple) and len(output) == 2 and getattr(output[0], 'ndim', 0) == 3:
        det, count = output
        output = [det[i, :max(min(int(c), det.shape[1]), 0)] for i, c in enumerate(count.tolist())]
    targets = []
    for i, o in enumerate(output):
        o = o.cpu().numpy() if isinstance(o, torch.Tensor) else np.asarray(o)
        for *box, conf, cls in o:
            x1, y1, x2, y2 = box
            targets.append([i, cls, (x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1, conf])
    return np.array(targets)


def _upload(arr, device):
    """A host array to the device from pinned memory, without waiting for it."""
    return torch.from_numpy(np.ascontiguousarray(arr)).pin_memory().to(device, non_blocking=True)


def _host_targets(targets, n_img, device):
    """The reference's host rows, grouped by image with a stable sort: [n, 6] labels -> ('labels', rows, label_off);
    [n, 7] predictions (x, y, w, h in pixels, conf last) -> ('pred', det [B, max_det, 6], count)."""
    t = targets.cpu().numpy() if isinstance(targets, torch.Tensor) else np.asarray(targets)
    t = np.asarray(t, np.float32)
    if t.ndim != 2 or t.shape[1] not in (6, 7):
        raise ValueError(f'plot_images: host targets must be [n, 6] or [n, 7], got {t.shape}')
    img = t[:, 0].astype(np.int64)
    t, img = t[(img >= 0) & (img < n_img)], img[(img >= 0) & (img < n_img)]
    order = np.argsort(img, kind='stable')
    t, img = t[order], img[order]
    per = np.bincount(img, minlength=n_img)
    off = np.concatenate(([0], np.cumsum(per))).astype(np.int32)
    if t.shape[1] == 6:
        return 'labels', _upload(t, device), _upload(off, device)
    max_det = max(int(per.max()) if len(per) else 0, 1)
    det = np.zeros((n_img, max_det, 6), np.float32)
    hw, hh = t[:, 4] / np.float32(2), t[:, 5] / np.float32(2)
    rows = np.stack([t[:, 2] - hw, t[:, 3] - hh, t[:, 2] + hw, t[:, 3] + hh, t[:, 6], t[:, 1]], 1)
    for b in range(n_img):
        det[b, :per[b]] = rows[off[b]:off[b + 1]]
    return 'pred', _upload(det, device), _upload(per.astype(np.int32), device)


def mosaic_tables(names, device, atlas=None):
    """(palette, (names blob, offsets, nc), atlas) on the device, as plot_images passes them on.  They are cached:
    the first use uploads them (and waits for that), so a caller that must not wait calls this ahead of time."""
    device = _hip_device(device)
    if isinstance(names, dict):   # {index: name}
        names = [names.get(i, str(i)) for i in range(max(names) + 1)] if names else None
    if atlas is None:
        atlas = glyph_atlas(text_height(L.MOSAIC_THICKNESS), device)
    return (_palette(color_list(), device), _names_blob(names if names else [str(i) for i in range(1024)], device),
            atlas)


def plot_images(images, targets, paths=None, fname='images.jpg', names=None, max_size=640, max_subplots=16, *,
                label_off=None, normalized=True, max_out=1280, atlas=None):
    """plot_images (plots.py:114-190) on the device: one yv7_mosaic call (four launches) builds the picture grid of
    the batch's first max_subplots images with boxes, captions and borders, downscaled to at most max_out pixels.

    images: HIP tensor [B, 3, H, W], uint8 or fp16 / fp32 in [0, 1].  targets: a (det, count) pair on the device
    (nms_batched's, in canvas pixels: predictions, drawn above conf 0.25 as 'name d.d'); a device [L, 6] tensor
    (image, class, x, y, w, h) sorted by image, with label_off [B + 1] (counted on the device if None), `normalized`
    saying whether xywh are fractions of the image or pixels: labels, drawn as 'name'; a host array or tensor in
    the reference's [n, 6] / [n, 7] format; or None / empty.  names=None labels with the class index.  paths: the
    captions, Path(p).name[:40].  The contract is in include/yv7.h; the picture is not cv2's.
    Returns the picture as a device uint8 [out_h, out_w, 3] tensor, stream-ordered; with fname it is also saved
    with PIL, the one host read (fname=None reads nothing back)."""
    if not (isinstance(images, torch.Tensor) and images.is_cuda):
        raise RuntimeError('plot_images draws on a ROCm device (libyv7); got CPU images')
    kinds = {torch.uint8: L.MOSAIC_U8, torch.float16: L.MOSAIC_F16, torch.float32: L.MOSAIC_F32}
    if images.dim() != 4 or images.shape[1] != 3 or images.dtype not in kinds or images.shape[0] == 0:
        raise ValueError(f'plot_images: expected uint8 / fp16 / fp32 images [B, 3, H, W], got {images.dtype} '
                         f'{tuple(images.shape)}')
    device = images.device
    images = images.contiguous()
    B, _, H, W = images.shape
    geo = mosaic_geometry(B, H, W, max_size, max_subplots, max_out)
    n = geo['n']

    d = L.MosaicDesc()
    d.images, d.in_kind, d.B, d.H, d.W = images.data_ptr(), kinds[images.dtype], B, H, W
    d.n, d.ns, (d.tile_h, d.tile_w), d.sf = n, geo['ns'], geo['tile'], geo['sf']
    d.out_h, d.out_w = geo['out']
    d.normalized = int(bool(normalized))
    keep = [images]

    kind = None
    if isinstance(targets, tuple):
        kind, (det, count) = 'pred', targets
    elif isinstance(targets, torch.Tensor) and targets.is_cuda:
        kind, rows = 'labels', targets
        if label_off is None:   # counted on the device: a comparison and a cumsum, nothing waits
            per = (rows[:, 0:1] == torch.arange(B, device=device, dtype=rows.dtype)).sum(0, dtype=torch.int32)
            label_off = torch.cat((torch.zeros(1, dtype=torch.int32, device=device), per.cumsum(0, dtype=torch.int32)))
    elif targets is not None and len(targets) > 0:
        kind, a, b = _host_targets(targets, B, device)
        if kind == 'pred':
            det, count = a, b
        else:
            rows, label_off = a, b
    if kind == 'pred':
        if det.dtype != torch.float32 or det.dim() != 3 or det.shape[0] != B or det.shape[2] != 6 or \
                not det.is_contiguous() or det.device != device:
            raise ValueError(f'plot_images: expected contiguous fp32 det [B, max_det, 6] for {B} images')
        if count.dtype != torch.int32 or tuple(count.shape) != (B,) or not count.is_contiguous() or \
                count.device != device:
            raise ValueError('plot_images: count must be int32 [B] on the images\' device')
        d.det, d.count, d.max_det = det.data_ptr(), count.data_ptr(), det.shape[1]
        keep += [det, count]
    elif kind == 'labels':
        if rows.dim() != 2 or rows.shape[1] != 6 or rows.device != device:
            raise ValueError(f'plot_images: expected labels [L, 6] on the images\' device, got {tuple(rows.shape)}')
        rows = rows.float().contiguous()
        if label_off.dtype != torch.int32 or tuple(label_off.shape) != (B + 1,) or not label_off.is_contiguous() or \
                label_off.device != device:
            raise ValueError('plot_images: label_off must be int32 [B + 1] on the images\' device')
        d.L, d.targets, d.label_off = rows.shape[0], rows.data_ptr() if rows.shape[0] else None, label_off.data_ptr()
        keep += [rows, label_off]

    pal, (blob, off, nc), atlas = mosaic_tables(names, device, atlas)
    d.palette, d.npal, d.names, d.name_off, d.nc = pal.data_ptr(), pal.shape[0], blob.data_ptr(), off.data_ptr(), nc
    d.atlas.metrics, d.atlas.cover = atlas.metrics.data_ptr(), atlas.cover.data_ptr()
    d.atlas.cell_h, d.atlas.total_w = atlas.cell_h, atlas.total_w
    if paths:
        from pathlib import Path
        raw = [Path(paths[i]).name[:40].encode('utf-8') if i < len(paths) else b'' for i in range(n)]
        cap_off = np.concatenate(([0], np.cumsum([len(r) for r in raw]))).astype(np.int32)
        caps = _upload(np.frombuffer(b''.join(raw) + b'\0', np.uint8).copy(), device)   # never empty
        cap_off_d = _upload(cap_off, device)
        d.captions, d.cap_off, d.cap_bytes = caps.data_ptr(), cap_off_d.data_ptr(), int(cap_off[-1])
        keep += [caps, cap_off_d]

    lib = L.lib()
    out = torch.empty((d.out_h, d.out_w, 3), dtype=torch.uint8, device=device)
    need = int(lib.yv7_mosaic_ws_bytes(ctypes.byref(d)))
    if need == 0:
        L.check(-1, 'yv7_mosaic_ws_bytes')
    ws = torch.empty(need, dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream(device).cuda_stream
        rc = lib.yv7_mosaic(ctypes.byref(d), out.data_ptr(), ws.data_ptr(), ws.numel(), stream)
    L.check(rc, 'yv7_mosaic')
    if fname:
        from PIL import Image
        Image.fromarray(out.cpu().numpy()).save(fname)
    return out
