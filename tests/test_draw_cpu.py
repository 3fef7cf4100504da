"""Drawing boxes on the device, the parts that need no GPU: the numpy restatement of the contract (tests/draw_ref.py)
against hand-worked pixel sets, the confidence digits against Python's own formatting, utils/plots.py's host-side
helpers, every validation message of yv7_draw_boxes, and detect.py's --save-img flag."""
import ctypes

import numpy as np
import pytest

import draw_ref as R
from utils import plots
from yv7 import _lib

RED = (200, 10, 20)


def _painted(img):
    """The set of (x, y) whose pixel is not zero."""
    ys, xs = np.nonzero(img.any(axis=2))
    return set(zip(xs.tolist(), ys.tolist()))


def _box(h, w, row, t, **kw):
    return R.draw(np.zeros((h, w, 3), np.uint8), [row], [RED], t, **kw)


# ------------------------------------------------------------------------------------------ the restatement
def test_outline_t1_t2_t3_by_hand():
    row = [3.9, 3.2, 8.7, 8.99, 0.5, 0.]        # truncates to (3, 3) - (8, 8)
    # t = 1: lo = 0, the bands are the lines x = 3, x = 8, y = 3, y = 8 between 3 and 8
    want1 = {(x, y) for x in range(3, 9) for y in range(3, 9) if x in (3, 8) or y in (3, 8)}
    assert len(want1) == 20
    # t = 2: lo = 1, bands [2, 3] and [7, 8], outer square 2 .. 8
    want2 = {(x, y) for x in range(2, 9) for y in range(2, 9) if x in (2, 3, 7, 8) or y in (2, 3, 7, 8)}
    assert len(want2) == 49 - 9
    # t = 3: lo = 1, bands [2, 4] and [7, 9], outer square 2 .. 9
    want3 = {(x, y) for x in range(2, 10) for y in range(2, 10) if x in (2, 3, 4, 7, 8, 9) or y in (2, 3, 4, 7, 8, 9)}
    assert len(want3) == 64 - 4
    for t, want in ((1, want1), (2, want2), (3, want3)):
        img = _box(12, 12, row, t)
        assert _painted(img) == want, t
        assert {tuple(img[y, x]) for x, y in want} == {RED}


def test_swapped_degenerate_outside_and_skipped_rows():
    a = _box(12, 12, [3, 3, 8, 8, 0.5, 0.], 1)
    assert np.array_equal(_box(12, 12, [8, 8, 3, 3, 0.5, 0.], 1), a)          # both corners swapped
    assert np.array_equal(_box(12, 12, [8, 3, 3, 8, 0.5, 0.], 1), a)          # x alone
    assert _painted(_box(12, 12, [5, 2, 5, 6, 0.5, 0.], 1)) == {(5, y) for y in range(2, 7)}   # xa == xb
    assert _painted(_box(12, 12, [5, 2, 5, 2, 0.5, 0.], 1)) == {(5, 2)}
    assert _painted(_box(12, 12, [5, 2, 5, 2, 0.5, 0.], 3)) == {(x, y) for x in (4, 5, 6) for y in (1, 2, 3)}
    for row in ([20, 20, 30, 30, 0.5, 0.], [-30, -30, -20, -20, 0.5, 0.], [3, 40, 8, 50, 0.5, 0.]):
        assert not _painted(_box(12, 12, row, 3)), row                        # fully outside
    # a box around the whole image leaves it untouched: only the outline is painted
    assert not _painted(_box(12, 12, [-5, -5, 20, 20, 0.5, 0.], 2))
    for bad in ([float('nan'), 3, 8, 8, 0.5, 0.], [3, 3, float('inf'), 8, 0.5, 0.], [3, 3, 8, 8, float('nan'), 0.],
                [3, 3, 8, 8, 0.5, -1.], [3, 3, 8, 8, 0.5, float('nan')]):
        assert not _painted(_box(12, 12, bad, 1)), bad
    # -0.7 truncates toward zero, to 0, not to -1
    assert _painted(_box(4, 4, [-0.7, -0.7, 2, 2, 0.5, 0.], 1)) == \
        {(x, y) for x in range(3) for y in range(3) if x in (0, 2) or y in (0, 2)}


def test_half_outside_each_edge():
    # left: x -3 .. 4 -> the left line is gone, top and bottom run from 0
    assert _painted(_box(12, 12, [-3, 2, 4, 6, 0.5, 0.], 1)) == \
        {(x, y) for x in range(0, 5) for y in range(2, 7) if x == 4 or y in (2, 6)}
    assert _painted(_box(12, 12, [8, 2, 15, 6, 0.5, 0.], 1)) == \
        {(x, y) for x in range(8, 12) for y in range(2, 7) if x == 8 or y in (2, 6)}
    assert _painted(_box(12, 12, [2, -3, 6, 4, 0.5, 0.], 1)) == \
        {(x, y) for x in range(2, 7) for y in range(0, 5) if y == 4 or x in (2, 6)}
    assert _painted(_box(12, 12, [2, 8, 6, 15, 0.5, 0.], 1)) == \
        {(x, y) for x in range(2, 7) for y in range(8, 12) if y == 8 or x in (2, 6)}


def test_painters_order_and_reverse():
    pal = [(10, 10, 10), (20, 20, 20)]
    det = [[2, 2, 6, 6, 0.5, 0.], [4, 4, 8, 8, 0.5, 1.]]
    fwd = R.draw(np.zeros((12, 12, 3), np.uint8), det, pal, 1)
    rev = R.draw(np.zeros((12, 12, 3), np.uint8), det, pal, 1, reverse=True)
    assert fwd[4, 6, 0] == 20 and fwd[6, 4, 0] == 20      # the crossings take the later box's colour
    assert rev[4, 6, 0] == 10 and rev[6, 4, 0] == 10
    assert _painted(fwd) == _painted(rev)
    assert fwd[2, 2, 0] == 10 and fwd[8, 8, 0] == 20 and R.draw(fwd, [], pal, 1) is not fwd


def test_label_by_hand_on_the_synthetic_atlas():
    metrics, cover = R.synthetic_atlas(cell_h=4)
    g = lambda ch: ord(ch) - 32
    assert metrics[g('a')].tolist()[1] == 2 and metrics[g('b')].tolist()[1] == 3 and metrics[g('c')].tolist()[1] == 5
    assert int(metrics[:, 1].sum()) == cover.shape[1] == 2 * 92 + 10
    colour = (100, 50, 0)
    # 'abc 0.50': 2 + 3 + 5 + 5 * 2 = 20 columns; box corner (5, 10): background x 5 .. 25, y 10 - 4 - 3 = 3 .. 10;
    # cells on rows 10 - 1 - 4 = 5 .. 8
    img = R.draw(np.zeros((16, 40, 3), np.uint8), [[5, 10, 30, 14, 0.5, 0.]], [colour], 1, names=[b'abc'],
                 atlas=(metrics, cover))
    assert R.label_text(b'abc', 0.5) == b'abc 0.50'
    bg = {(x, y) for x in range(5, 26) for y in range(3, 11)}
    outline = {(x, y) for x in range(5, 31) for y in range(10, 15) if x in (5, 30) or y in (10, 14)}
    assert _painted(img) == bg | outline
    assert tuple(img[4, 5]) == colour and tuple(img[9, 7]) == colour and tuple(img[3, 25]) == colour   # around the cells
    assert tuple(img[5, 5]) == colour and tuple(img[8, 6]) == colour                      # 'a': coverage 0
    # 'b': coverage 128 -> (128 * text + 127 * colour + 127) // 255
    assert tuple(img[5, 7]) == ((128 * 225 + 127 * 100 + 127) // 255, (128 * 255 + 127 * 50 + 127) // 255,
                                (128 * 255 + 127 * 0 + 127) // 255) == (163, 153, 128)
    assert tuple(img[8, 9]) == (163, 153, 128) and tuple(img[8, 10]) != (163, 153, 128)
    # 'c': checkerboard of 255 and 0 starting at x = 10, cell row 0 = image row 5
    assert tuple(img[5, 10]) == R.TEXT and tuple(img[5, 11]) == colour and tuple(img[6, 10]) == colour
    assert tuple(img[6, 11]) == R.TEXT and tuple(img[5, 14]) == R.TEXT
    # every other glyph: coverage 255 over its two columns, x = 15 .. 24; x = 25 is background
    assert all(tuple(img[y, x]) == R.TEXT for x in range(15, 25) for y in range(5, 9))
    # a class beyond the names gets the box alone; a non-ASCII byte draws as '?'
    bare = R.draw(np.zeros((16, 40, 3), np.uint8), [[5, 10, 30, 14, 0.5, 1.]], [colour], 1, names=[b'abc'],
                  atlas=(metrics, cover))
    assert _painted(bare) == outline
    a = R.draw(np.zeros((16, 40, 3), np.uint8), [[5, 10, 30, 14, 0.5, 0.]], [colour], 1, names=[b'\xc3'],
               atlas=(metrics, cover))
    b = R.draw(np.zeros((16, 40, 3), np.uint8), [[5, 10, 30, 14, 0.5, 0.]], [colour], 1, names=[b'?'],
               atlas=(metrics, cover))
    assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------ conf digits
def _text(n):
    return f'{n // 100}.{n // 10 % 10}{n % 10}'


def test_conf_digits_equal_python_formatting():
    for c, want in ((0.125, '0.12'), (0.375, '0.38'), (0.625, '0.62'), (0.875, '0.88'), (0.0, '0.00'), (1.0, '1.00')):
        assert _text(R.conf_digits(c)) == want == f'{c:.2f}'
    ties = [np.float32(k / 200) for k in range(1, 200, 2)] + [np.float32(0.005), np.float32(0.995)]
    near = []
    for v in ties:
        near += [v, np.nextafter(v, np.float32(0)), np.nextafter(v, np.float32(1))]
    rs = np.random.RandomState(5)
    for v in near + list(rs.rand(10000).astype(np.float32)):
        assert _text(R.conf_digits(v)) == f'{float(v):.2f}', float(v)
    assert R.conf_digits(-0.3) == 0 and R.conf_digits(1.7) == 100


# ------------------------------------------------------------------------------------------ utils/plots.py
def test_color_list_and_line_thickness():
    assert plots.color_list() == [(31, 119, 180), (255, 127, 14), (44, 160, 44), (214, 39, 40), (148, 103, 189),
                                  (140, 86, 75), (227, 119, 194), (127, 127, 127), (188, 189, 34), (23, 190, 207)]
    assert plots.line_thickness((1080, 810)) == 3 and plots.line_thickness((1080, 810, 3)) == 3
    assert plots.line_thickness((64, 48)) == 1
    assert [plots.text_height(t) for t in (1, 2, 3)] == [10, 19, 28]


def test_glyph_atlas_is_deterministic_and_consistent():
    for cell_h in (10, 28):
        metrics, cover = plots.glyph_atlas_host(cell_h)
        plots._ATLAS_HOST.clear()
        again = plots.glyph_atlas_host(cell_h)
        assert np.array_equal(metrics, again[0]) and np.array_equal(cover, again[1])
        assert metrics.shape == (95, 2) and metrics.dtype == np.int32 and cover.dtype == np.uint8
        assert int(metrics[:, 1].sum()) == cover.shape[1] and (metrics[:, 1] >= 1).all()
        assert np.array_equal(metrics[:, 0], np.concatenate([[0], np.cumsum(metrics[:, 1])[:-1]]))
        assert cover.shape[0] >= 1
        assert not cover[:, :metrics[0, 1]].any() and cover[:, metrics[ord('A') - 32, 0]:].any()   # ' ' is empty


# ------------------------------------------------------------------------------------------ the C ABI
def test_draw_boxes_validation_messages():
    L = _lib.lib()
    P = lambda v: ctypes.c_void_p(v)   # never followed
    ok_img, ok_atlas = (0x1000, 48, 64, 1, 0), (0x2000, 0x3000, 7, 400)

    def call(images=(ok_img,), atlases=(ok_atlas,), B=None, det=P(0x4000), cnt=P(0x5000), max_det=300, pal=P(0x6000),
             npal=10, names=P(0x7000), off=P(0x8000), nc=80, n_atlas=None, ws=P(0x10000), ws_bytes=1 << 30):
        im = (_lib.DrawImage * max(len(images), 1))(*[_lib.DrawImage(*d) for d in images])
        at = (_lib.GlyphAtlas * max(len(atlases), 1))(*[_lib.GlyphAtlas(*d) for d in atlases])
        rc = L.yv7_draw_boxes(im if images else None, len(images) if B is None else B, det, cnt, max_det, pal, npal,
                              names, off, nc, at if atlases else None, len(atlases) if n_atlas is None else n_atlas,
                              0, ws, ws_bytes, None)
        return rc, L.yv7_last_error().decode()

    assert L.yv7_draw_ws_bytes(2, 300) == 2 * 300 * 48 and L.yv7_draw_ws_bytes(0, 300) == 0
    for args, code, text in [
        (dict(B=0), -1, 'B must be positive'),
        (dict(max_det=0), -1, 'max_det must be positive'),
        (dict(npal=0), -1, 'npal must be at least 1'),
        (dict(images=()), -1, 'B must be positive'),
        (dict(images=(), B=1), -1, 'null argument'),
        (dict(det=None), -1, 'null argument'),
        (dict(cnt=None), -1, 'null argument'),
        (dict(pal=None), -1, 'null argument'),
        (dict(ws=None), -1, 'null argument'),
        (dict(ws_bytes=300 * 48 - 1), -3, 'workspace too small'),
        (dict(ws=P(0x10008)), -1, 'ws must be 16-byte aligned'),
        (dict(off=None), -1, 'names without name_off or atlases'),
        (dict(atlases=()), -1, 'names without name_off or atlases'),
        (dict(nc=0), -1, 'nc must be at least 1'),
        (dict(n_atlas=0), -1, 'n_atlas must be in 1..8'),
        (dict(atlases=(ok_atlas,) * 9), -1, 'n_atlas must be in 1..8'),
        (dict(atlases=(ok_atlas, (0, 0x3000, 7, 400))), -1, 'atlas 1 has a null pointer'),
        (dict(atlases=((0x2000, 0, 7, 400),)), -1, 'atlas 0 has a null pointer'),
        (dict(atlases=((0x2000, 0x3000, 0, 400),)), -2, 'atlas 0 has a non-positive size'),
        (dict(atlases=((0x2000, 0x3000, 7, -1),)), -2, 'atlas 0 has a non-positive size'),
        (dict(images=(ok_img, (0, 48, 64, 1, 0))), -1, 'image 1 has null data'),
        (dict(images=((0x1000, 0, 64, 1, 0),)), -2, 'image 0 has a non-positive size'),
        (dict(images=((0x1000, 48, -3, 1, 0),)), -2, 'image 0 has a non-positive size'),
        (dict(images=((0x1000, (1 << 20) + 1, 64, 1, 0),)), -2, 'image 0 is too large'),
        (dict(images=(ok_img, ok_img, (0x1000, 48, 64, 0, 0))), -1, 'image 2: thickness must be in 1..4096'),
        (dict(images=((0x1000, 48, 64, 1, 1),)), -1, 'image 0: atlas index out of range'),
        (dict(images=((0x1000, 48, 64, 1, -1),)), -1, 'image 0: atlas index out of range'),
        (dict(images=((0x1000, 48, 64, 1, 2),), atlases=(ok_atlas, ok_atlas)), -1, 'image 0: atlas index out of range'),
    ]:
        rc, msg = call(**args)
        assert rc == code and msg.startswith('yv7_draw_boxes: ') and text in msg, (args, rc, msg)


def test_binding_mirrors_the_header():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'yv7.h')).read()
    for name, value in (('MAX_ATLAS', _lib.DRAW_MAX_ATLAS), ('TILE_W', _lib.DRAW_TILE_W), ('TILE_H', _lib.DRAW_TILE_H)):
        assert int(re.search(rf'#define YV7_DRAW_{name} (\d+)', hdr).group(1)) == value
    assert ctypes.sizeof(_lib.DrawImage) == 24 and ctypes.sizeof(_lib.GlyphAtlas) == 24
    assert re.search(r'#define YV7_ABI_VERSION 5\b', hdr) and _lib.ABI_VERSION == 5


# ------------------------------------------------------------------------------------------ detect.py
def test_detect_knows_save_img_and_it_is_off_by_default():
    import detect
    assert detect.parse_opt([]).save_img is False
    assert detect.parse_opt(['--save-img']).save_img is True


def test_plot_boxes_refuses_cpu_detections():
    import torch
    with pytest.raises(RuntimeError, match='ROCm device'):
        plots.plot_boxes([np.zeros((4, 4, 3), np.uint8)], torch.zeros(1, 1, 6), torch.zeros(1, dtype=torch.int32))
