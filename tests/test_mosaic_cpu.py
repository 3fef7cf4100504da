"""The picture grid (yv7_mosaic, utils.plots.plot_images), the parts that need no GPU: the geometry against the
reference's known answers, the numpy restatement of the contract (tests/mosaic_ref.py) against hand-worked pictures,
the confidence digit against Python's own formatting, the 0.25 threshold, every validation message of yv7_mosaic,
the host half of utils/plots.py and the binding against the header."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import draw_ref as R
import mosaic_ref as M
from utils import plots
from yv7 import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------ geometry
@pytest.mark.parametrize('args, kw, ns, tile, mosaic, out', [
    ((32, 640, 640), {}, 4, (640, 640), (2560, 2560), (1280, 1280)),
    ((8, 1280, 1280), {}, 3, (640, 640), (1920, 1920), (1280, 1280)),
    ((32, 480, 640), {}, 4, (480, 640), (1920, 2560), (960, 1280)),
    ((5, 384, 640), {}, 3, (384, 640), (1152, 1920), (768, 1280)),
    ((32, 672, 1280), {}, 4, (336, 640), (1344, 2560), (672, 1280)),
    ((1, 640, 640), {}, 1, (640, 640), (640, 640), (640, 640)),
    ((3, 100, 70), dict(max_size=48), 2, (48, 34), (96, 68), (96, 68)),
])
def test_geometry_known_answers(args, kw, ns, tile, mosaic, out):
    g = plots.mosaic_geometry(*args, **kw)
    assert (g['ns'], g['tile'], g['mosaic'], g['out']) == (ns, tile, mosaic, out)
    assert g['n'] == min(args[0], 16) and len(g['blocks']) == g['n']


def test_geometry_clamps_to_sixteen_and_fills_columns_first():
    g = plots.mosaic_geometry(17, 64, 48)
    assert g['n'] == 16 and g['ns'] == 4 and g['sf'] == 10.0 and g['tile'] == (64, 48)
    assert g['blocks'][:5] == [(0, 0), (0, 64), (0, 128), (0, 192), (48, 0)] and g['blocks'][15] == (144, 192)
    g = plots.mosaic_geometry(2, 64, 48)
    assert g['n'] == 2 and g['ns'] == 2 and g['blocks'] == [(0, 0), (0, 64)] and g['mosaic'] == (128, 96)
    g = plots.mosaic_geometry(5, 10, 10, max_subplots=4)
    assert g['n'] == 4 and g['ns'] == 2
    # max_out reaches the downscale at small shapes: r = 60 / 40 / 2 = 0.75
    g = plots.mosaic_geometry(4, 40, 30, max_out=60)
    assert g['mosaic'] == (80, 60) and g['out'] == (60, 45)
    assert M.block(3, 2, 40, 30) == (30, 40) == g['blocks'][3]


# ------------------------------------------------------------------------------------------ the restatement
COLOURS = [(10, 20, 30), (40, 50, 60), (70, 80, 90), (100, 110, 120)]


def _constant_tiles(n, h=4, w=6):
    img = np.zeros((n, 3, h, w), np.uint8)
    for i in range(n):
        for c in range(3):
            img[i, c] = COLOURS[i][c]
    return img


def test_two_by_two_grid_by_hand():
    """4 x 6 tiles on an 8 x 12 mosaic: the lines x = 0, 6, 12 and y = 0, 4, 8 with their neighbours are white,
    which leaves columns 2-4 and 8-10 of rows 2 and 6; tile i sits in column i // 2, row i % 2."""
    got = M.mosaic(_constant_tiles(4), 4, 2, 4, 6, 160.0, 8, 12)
    W = (255, 255, 255)
    c0, c1, c2, c3 = COLOURS
    white_row = [W] * 12
    upper = [W, W, c0, c0, c0, W, W, W, c2, c2, c2, W]
    lower = [W, W, c1, c1, c1, W, W, W, c3, c3, c3, W]
    want = np.array([white_row, white_row, upper, white_row, white_row, white_row, lower, white_row], np.uint8)
    assert np.array_equal(got, want)
    # before the borders every block position holds its tile
    img = np.full((8, 12, 3), 255, np.uint8)
    for i in range(4):
        bx, by = M.block(i, 2, 4, 6)
        assert (bx, by) == [(0, 0), (0, 4), (6, 0), (6, 4)][i]
        img[by:by + 4, bx:bx + 6] = COLOURS[i]
        M.paint_border(img, bx, by, 4, 6)
    assert np.array_equal(img, want)
    # two tiles: column 0 alone; column 1 stays canvas, and only tile borders are drawn
    two = M.mosaic(_constant_tiles(2), 2, 2, 4, 6, 160.0, 8, 12)
    want2 = want.copy()
    want2[:, 6:] = 255
    assert np.array_equal(two, want2)
    # one 6 x 8 tile: the border band is the outer two pixels on the left / top, one on the right / bottom
    one = M.mosaic(_constant_tiles(1, 6, 8), 1, 1, 6, 8, 80.0, 6, 8)
    inner = np.zeros((6, 8), bool)
    inner[2:5, 2:7] = True
    assert np.array_equal((one == np.array(COLOURS[0], np.uint8)).all(2), inner) and (one[~inner] == 255).all()


def test_area_weights_by_hand():
    assert M.area_weights(3, 2).tolist() == [[2, 1, 0], [0, 1, 2]]
    assert M.area_weights(4, 2).tolist() == [[2, 2, 0, 0], [0, 0, 2, 2]]
    assert M.area_weights(5, 5).tolist() == (5 * np.eye(5, dtype=int)).tolist()
    s3 = np.array([[0, 9, 18], [27, 36, 45], [54, 63, 72]], np.uint8)
    got = M.area_resize(np.stack([s3, s3, 255 - s3], 2), 2, 2)
    # (4 * 0 + 2 * 9 + 2 * 27 + 36 + 4) // 9 = 12, (2 * 9 + 4 * 18 + 36 + 2 * 45 + 4) // 9 = 24, ...
    assert got[:, :, 0].tolist() == [[12, 24], [48, 60]] == got[:, :, 1].tolist()
    assert got[:, :, 2].tolist() == [[243, 231], [207, 195]]
    s4 = np.array([[1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11, 13], [13, 14, 15, 18]], np.uint8)
    got = M.area_resize(np.stack([s4] * 3, 2), 2, 2)
    assert got[:, :, 0].tolist() == [[(1 + 2 + 5 + 6 + 2) >> 2, (3 + 4 + 7 + 8 + 2) >> 2],
                                     [(9 + 10 + 13 + 14 + 2) >> 2, (11 + 13 + 15 + 18 + 2) >> 2]] == [[4, 6], [12, 14]]
    same = M.area_resize(np.stack([s4] * 3, 2), 4, 4)
    assert np.array_equal(same[:, :, 0], s4)
    # a constant picture stays constant at a ratio with remainders
    assert (M.area_resize(np.full((97, 81, 3), 201, np.uint8), 33, 27) == 201).all()


def test_caption_blend_at_coverage_0_128_255():
    atlas = R.synthetic_atlas(cell_h=2)
    img = np.full((12, 20, 3), 100, np.uint8)
    img[:, :, 2] = 0
    M.paint_caption(img, b'abd\xc3', 1, 2, atlas)     # pen 6, rows 7 .. 8: 'a' 6-7, 'b' 8-10, 'd' 11-12, '?' 13-14
    mid = ((128 * 220 + 127 * 100 + 127) // 255, (128 * 220 + 127 * 0 + 127) // 255)
    assert mid == (160, 110)
    for y in (7, 8):
        assert [tuple(p) for p in img[y, 5:16]] == [(100, 100, 0)] * 3 + [(mid[0], mid[0], mid[1])] * 3 + \
            [(220, 220, 220)] * 4 + [(100, 100, 0)]
    assert (img[6] == (100, 100, 0)).all() and (img[9] == (100, 100, 0)).all()
    # clipped at the right edge and below
    img = np.full((8, 8, 3), 50, np.uint8)
    M.paint_caption(img, b'dddd', 0, 2, atlas)        # pen 5, rows 7 .. 8 -> row 7, columns 5 .. 7 only
    assert (img[7, 5:] == 220).all() and (img[:7] == 50).all() and (img[7, :5] == 50).all()


def test_pred_label_digit_equals_python_formatting():
    for c, want in ((0.05, '0.1'), (0.15, '0.2'), (0.25, '0.2'), (0.949999, '0.9'), (0.95, '0.9'), (1.0, '1.0')):
        v = np.float32(c)
        n = M.conf_digit(v)
        assert f'{n // 10}.{n % 10}' == '%.1f' % float(v) == want, c
    ties = [np.float32(k / 20) for k in range(1, 20, 2)]
    near = []
    for v in ties:
        near += [v, np.nextafter(v, np.float32(0)), np.nextafter(v, np.float32(1))]
    for v in near + list(np.random.RandomState(3).rand(5000).astype(np.float32)):
        n = M.conf_digit(v)
        assert f'{n // 10}.{n % 10}' == '%.1f' % float(v), float(v)
    assert M.conf_digit(-1.0) == 0 and M.conf_digit(7.0) == 10
    assert M.pred_label(b'bus', 0.949999) == b'bus 0.9' and M.pred_label(b'', 1.0) == b' 1.0'


def test_threshold_is_strict_and_rows_are_fp32():
    up = np.nextafter(np.float32(0.25), np.float32(1))
    det = np.zeros((2, 3, 6), np.float32)
    det[0, 0] = [1, 2, 3, 4, 0.25, 0]
    det[0, 1] = [1, 2, 3, 4, up, 1]
    det[0, 2] = [1, 2, 3, 4, 0.9, 2]          # beyond count
    det[1, 0] = [1.5, 2.5, 3.5, 4.5, 0.5, 3]
    rows = M.pred_rows(det, [2, 7], 2, 2, 10, 20, 2.0)
    assert rows[:, 5].tolist() == [1, 3]     # image 1: count clamps to max_det, and its zero rows fail conf
    det[1, 2, 4:] = [0.3, 4]
    assert M.pred_rows(det, [2, 7], 2, 2, 10, 20, 2.0)[:, 5].tolist() == [1, 3, 4]
    det[1, 2] = 0
    rows = M.pred_rows(det, [2, 1], 2, 2, 10, 20, 2.0)
    assert rows.tolist() == [[1, 2, 3, 4, up, 1], [1.5, 12.5, 3.5, 14.5, 0.5, 3]]     # tile 1 sits at (0, 10)
    rows = M.pred_rows(det, [-4, 1], 2, 2, 10, 20, 0.3)
    s = np.float32(0.3)
    assert rows.dtype == np.float32 and rows[0, :4].tolist() == [np.float32(1.5) * s, np.float32(2.5) * s + np.float32(10),
                                                                 np.float32(3.5) * s, np.float32(4.5) * s + np.float32(10)]
    t = np.array([[0, 5, .5, .5, .2, .4], [1, 6, .5, .5, 1, 1], [1, 7, 8, 8, 4, 4]], np.float32)
    rows = M.label_rows(t, [0, 1, 3], 2, 2, 10, 20, 0.5, True)
    f = np.float32
    assert rows[0].tolist() == [(f(.5) - f(.1)) * f(20), (f(.5) - f(.2)) * f(10), (f(.5) + f(.1)) * f(20),
                                (f(.5) + f(.2)) * f(10), 1, 5]
    assert rows[1].tolist() == [0, 10, 20, 20, 1, 6]
    rows = M.label_rows(t, [0, 1, 3], 2, 2, 10, 20, 0.5, False)
    assert rows[2].tolist() == [3, 13, 5, 15, 1, 7]
    assert len(M.label_rows(t, [0, 1, 3], 1, 2, 10, 20, 0.5, False)) == 1      # image 1 is no tile


# ------------------------------------------------------------------------------------------ the C ABI
def _desc(**kw):
    d = _lib.MosaicDesc()
    base = dict(images=0x1000, in_kind=0, B=4, H=40, W=56, n=4, ns=2, tile_h=40, tile_w=56, sf=1.0, det=0x2000,
                count=0x3000, max_det=300, L=0, targets=None, label_off=None, normalized=1, npal=10, palette=0x4000,
                names=0x5000, name_off=0x6000, nc=80, cap_bytes=10, captions=0x7000, cap_off=0x8000, out_h=80,
                out_w=112)
    base.update(kw)
    atlas = base.pop('atlas', (0x9000, 0xa000, 7, 400))
    for k, v in base.items():
        setattr(d, k, v)
    d.atlas = _lib.GlyphAtlas(*atlas)
    return d


def test_mosaic_validation_messages():
    L = _lib.lib()
    ok = _desc()
    canvas = 80 * 112 * 3
    assert L.yv7_mosaic_ws_bytes(ctypes.byref(ok)) == 4 * 300 * 48 + canvas
    assert L.yv7_mosaic_ws_bytes(ctypes.byref(_desc(det=None, count=None))) == canvas
    labels = dict(det=None, count=None, label_off=0x2000, targets=0x3000, L=3)
    assert L.yv7_mosaic_ws_bytes(ctypes.byref(_desc(**labels))) == 3 * 48 + canvas
    assert L.yv7_mosaic_ws_bytes(ctypes.byref(_desc(**{**labels, 'L': 0, 'targets': None}))) == canvas
    assert L.yv7_mosaic_ws_bytes(None) == 0 and L.yv7_mosaic_ws_bytes(ctypes.byref(_desc(n=5))) == 0

    def call(d, out=0x100000, ws=0x200000, ws_bytes=1 << 30):
        rc = L.yv7_mosaic(ctypes.byref(d) if d is not None else None, out, ws, ws_bytes, None)
        return rc, L.yv7_last_error().decode()

    for args, code, text in [
        (dict(images=None), -1, 'null images'),
        (dict(in_kind=3), -1, 'in_kind must be'),
        (dict(in_kind=-1), -1, 'in_kind must be'),
        (dict(B=0), -2, 'B, H and W must be positive'),
        (dict(H=-1), -2, 'B, H and W must be positive'),
        (dict(W=(1 << 20) + 1), -2, 'an image side above 2^20'),
        (dict(n=0), -2, 'n, ns, tile_h and tile_w must be positive'),
        (dict(tile_w=0), -2, 'n, ns, tile_h and tile_w must be positive'),
        (dict(n=5, B=8, ns=2), -2, 'n exceeds ns * ns'),
        (dict(n=4, B=3), -2, 'n exceeds B'),
        (dict(ns=128, tile_w=129), -2, 'the mosaic is too large'),
        (dict(ns=4, tile_h=4097), -2, 'the mosaic is too large'),
        (dict(sf=0.0), -1, 'sf must be positive'),
        (dict(sf=float('nan')), -1, 'sf must be positive'),
        (dict(out_h=0), -2, 'out_h and out_w must be positive'),
        (dict(out_h=81), -2, 'the output is larger than the mosaic'),
        (dict(out_w=113), -2, 'the output is larger than the mosaic'),
        (dict(out_h=9), -2, 'the output is more than 8 times smaller than the mosaic'),
        (dict(out_w=13), -2, 'the output is more than 8 times smaller than the mosaic'),
        (dict(label_off=0x2000), -1, 'predictions and labels both given'),
        (dict(targets=0x2000), -1, 'predictions and labels both given'),
        (dict(count=None), -1, 'det without count'),
        (dict(max_det=0), -1, 'max_det must be positive'),
        (dict(max_det=1 << 23), -2, 'more than 2^24 rows'),
        ({**labels, 'L': -1}, -2, 'L must be in'),
        ({**labels, 'targets': None}, -1, 'label_off without targets'),
        ({**labels, 'label_off': None}, -1, 'targets without label_off'),
        (dict(palette=None), -1, 'rows without a palette'),
        (dict(npal=0), -1, 'npal must be at least 1'),
        (dict(name_off=None), -1, 'names without name_off'),
        (dict(nc=0), -1, 'nc must be at least 1'),
        (dict(captions=None), -1, 'captions and cap_off go together'),
        (dict(cap_off=None), -1, 'captions and cap_off go together'),
        (dict(cap_bytes=-1), -1, 'cap_bytes must not be negative'),
        (dict(atlas=(0, 0xa000, 7, 400)), -1, 'the atlas has a null pointer'),
        (dict(atlas=(0x9000, 0xa000, 0, 400)), -2, 'the atlas has a non-positive size'),
        (dict(atlas=(0x9000, 0xa000, 7, 0), names=None), -2, 'the atlas has a non-positive size'),
    ]:
        rc, msg = call(_desc(**args))
        assert rc == code and msg.startswith('yv7_mosaic: ') and text in msg, (args, rc, msg)
    # without names and captions no atlas is needed: the call gets as far as its own arguments
    bare = _desc(names=None, captions=None, cap_off=None, atlas=(0, 0, 0, 0))
    for kw, code, text in [(dict(out=None), -1, 'null argument'), (dict(ws=None), -1, 'null argument'),
                           (dict(ws_bytes=4 * 300 * 48 + canvas - 1), -3, 'workspace too small'),
                           (dict(ws=0x200008), -1, 'ws must be 16-byte aligned')]:
        rc, msg = call(bare, **kw)
        assert rc == code and msg.startswith('yv7_mosaic: ') and text in msg, (kw, rc, msg)
    rc, msg = call(None)
    assert rc == -1 and msg == 'yv7_mosaic: null argument'


def test_binding_mirrors_the_header(tmp_path):
    hdr = open(os.path.join(ROOT, 'include', 'yv7.h')).read()
    for name, value in (('U8', _lib.MOSAIC_U8), ('F16', _lib.MOSAIC_F16), ('F32', _lib.MOSAIC_F32),
                        ('MAX_SIDE', _lib.MOSAIC_MAX_SIDE), ('THICKNESS', _lib.MOSAIC_THICKNESS),
                        ('MAX_RATIO', _lib.MOSAIC_MAX_RATIO)):
        assert int(re.search(rf'#define YV7_MOSAIC_{name} (\d+)', hdr).group(1)) == value
    assert re.search(r'#define YV7_ABI_VERSION 5\b', hdr) and _lib.ABI_VERSION == 5
    for name in ('yv7_mosaic', 'yv7_mosaic_ws_bytes'):
        assert name in _lib.SIGNATURES and hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    fields = [f[0] for f in _lib.MosaicDesc._fields_]
    prog = tmp_path / 'layout.c'
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "yv7.h"\nint main(void){'
                    'printf("%zu", sizeof(yv7_mosaic_desc));'
                    + ''.join(f'printf(" %zu", offsetof(yv7_mosaic_desc, {f}));' for f in fields)
                    + 'printf("\\n");return 0;}\n')
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(prog), '-o', str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(_lib.MosaicDesc)] + [getattr(_lib.MosaicDesc, f).offset for f in fields]
    assert got[0] == 176


# ------------------------------------------------------------------------------------------ utils/plots.py
def test_plot_images_refuses_cpu_images():
    with pytest.raises(RuntimeError, match='ROCm device'):
        plots.plot_images(torch.zeros(1, 3, 8, 8), None, fname=None)
    with pytest.raises(RuntimeError, match='ROCm device'):
        plots.plot_images(np.zeros((1, 3, 8, 8), np.float32), None, fname=None)


def test_output_to_target_by_hand():
    out = [torch.tensor([[10., 20., 30., 60., 0.9, 2.], [0., 0., 4., 2., 0.3, 7.]]), torch.zeros(0, 6),
           torch.tensor([[1., 1., 2., 3., 0.5, 0.]])]
    want = [[0, 2, 20, 40, 20, 40, 0.9], [0, 7, 2, 1, 4, 2, 0.3], [2, 0, 1.5, 2, 1, 2, 0.5]]
    got = plots.output_to_target(out)
    assert got.shape == (3, 7) and np.allclose(got, np.array(want), rtol=0, atol=1e-7)
    det = torch.zeros(3, 2, 6)
    det[0], det[2, 0] = out[0], out[2][0]
    det[1, 0] = torch.tensor([5., 5., 6., 6., 0.8, 1.])        # beyond count[1] = 0
    pair = plots.output_to_target((det, torch.tensor([2, 0, 1], dtype=torch.int32)))
    assert np.array_equal(pair, got)
    assert plots.output_to_target([]).shape == (0,)


def test_host_targets_are_grouped_by_image_with_a_stable_sort(monkeypatch):
    monkeypatch.setattr(plots, '_upload', lambda arr, device: np.array(arr))
    t = np.array([[1, 5, .5, .5, .2, .2], [0, 6, .1, .1, .1, .1], [1, 7, .3, .3, .1, .1], [9, 1, 0, 0, 0, 0]], np.float32)
    kind, rows, off = plots._host_targets(t, 3, None)
    assert kind == 'labels' and rows[:, 1].tolist() == [6, 5, 7] and off.tolist() == [0, 1, 3, 3]
    p = np.array([[1, 5, 10, 10, 4, 2, .9], [0, 6, 3, 3, 2, 2, .8], [1, 7, 1, 1, 2, 2, .7]], np.float32)
    kind, det, count = plots._host_targets(p, 2, None)
    assert kind == 'pred' and det.shape == (2, 2, 6) and count.tolist() == [1, 2]
    assert det[1].tolist() == [[8, 9, 12, 11, np.float32(.9), 5], [0, 0, 2, 2, np.float32(.7), 7]]
    assert det[0, 0].tolist() == [2, 2, 4, 4, np.float32(.8), 6] and not det[0, 1].any()
