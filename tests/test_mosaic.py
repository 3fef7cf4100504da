"""yv7_mosaic through the C ABI against the numpy restatement of its contract (tests/mosaic_ref.py), bit for bit, on
random-noise images with the synthetic atlas.  The output and the workspace sit inside larger buffers whose guard
bytes are checked afterwards.  Shapes are the smallest at which each piece can go wrong: tile counts around the
grid sizes, tiles around the pixel kernel's 64 x 32 tile, each resize mode, each kind of output ratio."""
import ctypes

import numpy as np
import pytest
import torch

import draw_ref as R
import mosaic_ref as M
from utils import plots
from yv7 import _lib

pytestmark = pytest.mark.gpu

GUARD = 4096
PALETTE = [(200, 10, 20), (10, 220, 30), (20, 30, 240)]
NAMES = [b'a', b'abc', b'a name of thirty characters ..', b'caf\xe9', b'']
ATLAS = R.synthetic_atlas(cell_h=4)
SPECIAL = [0.0, 1.0, float('nan'), -0.1, 1.2]


def _images(rs, B, H, W, kind):
    u8 = rs.randint(0, 256, (B, 3, H, W)).astype(np.uint8)
    if kind == 'u8':
        return u8
    x = (u8.astype(np.float32) / np.float32(255) + rs.rand(B, 3, H, W).astype(np.float32) / 300).astype(
        np.float16 if kind == 'f16' else np.float32)
    for b, c, y, x0 in _special_places(B, H, W):
        x[b, c, y, x0:x0 + len(SPECIAL)] = SPECIAL
    return x


def _special_places(B, H, W):
    """(image, channel, row, first column) of each run of SPECIAL: the middle rows of image 0, one run per channel,
    away from the border band, so that every value reaches the compared picture (identity, 2x and bilinear tiles)."""
    return [(0, c, H // 2 + c, W // 2 - 3 + c) for c in range(3)]


def _assert_specials_are_seen(images, *geometry):
    """The reference picture changes when any one of the special values is replaced: the comparison sees each."""
    want = M.mosaic(images, *geometry)
    B, _, H, W = images.shape
    for k, v in enumerate(SPECIAL):
        other = images.copy()
        for b, c, y, x0 in _special_places(B, H, W):
            other[b, c, y, x0 + k] = 0.5 if v != 1.2 else 0.25     # 1.2 and 0.5 + noise may both clamp near
        assert not np.array_equal(M.mosaic(other, *geometry), want), v
    nan_high = images.copy()
    nan_high[np.isnan(nan_high)] = 1.0                              # NaN -> 255 would show
    assert not np.array_equal(M.mosaic(nan_high, *geometry), want)


def run(images, n, ns, tile, sf, out, det=None, count=None, targets=None, label_off=None, normalized=True,
        names=NAMES, captions=None, atlas=ATLAS):
    """One yv7_mosaic call; returns (device picture, reference picture) after checking the guards and the inputs."""
    lib = _lib.lib()
    dev = torch.device('cuda', torch.cuda.current_device())
    rs = np.random.RandomState(11)
    keep = []

    def up(a):
        keep.append(torch.from_numpy(np.ascontiguousarray(a)).to(dev))
        return keep[-1]

    d = _lib.MosaicDesc()
    B, _, H, W = images.shape
    d.images = up(images).data_ptr()
    d.in_kind = {np.dtype(np.uint8): 0, np.dtype(np.float16): 1, np.dtype(np.float32): 2}[images.dtype]
    d.B, d.H, d.W, d.n, d.ns, (d.tile_h, d.tile_w), d.sf, (d.out_h, d.out_w) = B, H, W, n, ns, tile, sf, out
    d.normalized = int(normalized)
    det_t = None
    if det is not None:
        det_t = up(np.asarray(det, np.float32))
        d.det, d.count, d.max_det = det_t.data_ptr(), up(np.asarray(count, np.int32)).data_ptr(), det_t.shape[1]
    elif label_off is not None:
        t = np.asarray(targets, np.float32).reshape(-1, 6)
        d.L, d.label_off = len(t), up(np.asarray(label_off, np.int32)).data_ptr()
        d.targets = up(t).data_ptr() if len(t) else None
    pal = plots._palette(PALETTE, dev)
    d.palette, d.npal = pal.data_ptr(), pal.shape[0]
    if names is not None:
        blob, off, nc = plots._names_blob(names, dev)
        d.names, d.name_off, d.nc = blob.data_ptr(), off.data_ptr(), nc
    dev_atlas = plots.Atlas(*atlas, dev)
    d.atlas = _lib.GlyphAtlas(dev_atlas.metrics.data_ptr(), dev_atlas.cover.data_ptr(), dev_atlas.cell_h,
                              dev_atlas.total_w)
    if captions is not None:
        assert len(captions) == n
        cap_off = np.concatenate(([0], np.cumsum([len(c) for c in captions]))).astype(np.int32)
        d.captions = up(np.frombuffer(b''.join(captions) + b'\0', np.uint8).copy()).data_ptr()
        d.cap_off, d.cap_bytes = up(cap_off).data_ptr(), int(cap_off[-1])

    need = lib.yv7_mosaic_ws_bytes(ctypes.byref(d))
    assert need >= ns * tile[0] * ns * tile[1] * 3, lib.yv7_last_error()
    ws = torch.from_numpy(rs.randint(0, 256, 2 * GUARD + need).astype(np.uint8)).to(dev)
    ob = torch.from_numpy(rs.randint(0, 256, 2 * GUARD + out[0] * out[1] * 3).astype(np.uint8)).to(dev)
    ws0, ob0 = ws.cpu(), ob.cpu()
    rc = lib.yv7_mosaic(ctypes.byref(d), ob.data_ptr() + GUARD, ws.data_ptr() + GUARD, need,
                        torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, 'yv7_mosaic')
    torch.cuda.synchronize()
    ws1, ob1 = ws.cpu(), ob.cpu()
    for a, b in ((ws0, ws1), (ob0, ob1)):
        assert torch.equal(a[:GUARD], b[:GUARD]) and torch.equal(a[-GUARD:], b[-GUARD:]), 'a guard byte changed'
    if det_t is not None:   # read-only (bitwise: a NaN row is not equal to itself)
        assert np.array_equal(det_t.cpu().numpy().view(np.int32), np.asarray(det, np.float32).view(np.int32))
    got = ob1[GUARD:-GUARD].numpy().reshape(out[0], out[1], 3)
    want = M.mosaic(images, n, ns, tile[0], tile[1], sf, out[0], out[1], det=det, count=count, targets=targets,
                    label_off=label_off, normalized=normalized, palette=PALETTE, names=names, atlas=atlas,
                    captions=captions)
    if not np.array_equal(got, want):
        bad = np.argwhere((got != want).any(axis=2))
        raise AssertionError(f'{len(bad)} pixels differ, first (y, x) {bad[:5].tolist()} got {got[tuple(bad[0])]} '
                             f'want {want[tuple(bad[0])]}')
    return got, want


# ------------------------------------------------------------------------------------------ tiles and output
@pytest.mark.parametrize('B, n, ns, shape, tile, sf, out, kind', [
    (1, 1, 1, (40, 56), (40, 56), 1.4, (40, 56), 'u8'),              # one tile, a copy
    (2, 2, 2, (33, 65), (33, 65), 1.2, (66, 130), 'f16'),            # column 0 alone; odd width, one past the tile
    (4, 4, 2, (32, 64), (32, 64), 1.0, (32, 64), 'f32'),             # the pixel kernel's tile exactly; exact 2x out
    (5, 5, 3, (7, 5), (7, 5), 3.0, (21, 15), 'u8'),                  # ns = 3: a partial middle column, an empty last
    (16, 16, 4, (80, 112), (40, 56), 0.5, (80, 112), 'f16'),         # exact 2x tiles and exact 2x out
    (16, 16, 4, (80, 112), (40, 56), 0.5, (160, 224), 'u8'),
    (17, 16, 4, (24, 30), (24, 30), 2.0, (64, 80), 'u8'),            # B = 17 -> 16 tiles; 96 x 120 -> 3:2
    (1, 1, 1, (97, 81), (97, 81), 1.0, (33, 27), 'f32'),             # remainders in both axes
    (3, 3, 2, (100, 70), (48, 34), 0.48, (96, 68), 'u8'),            # bilinear: 102 values, both rounding branches
    (3, 3, 2, (100, 70), (48, 34), 0.48, (41, 29), 'f32'),
    (3, 3, 2, (100, 70), (48, 34), 0.48, (96, 68), 'f16'),
])
def test_gpu_mosaic_tiles_and_output(B, n, ns, shape, tile, sf, out, kind):
    """No rows, no captions: canvas, tiles of each input kind and resize mode, borders, each output ratio."""
    if tile != shape and kind == 'u8' and shape == (100, 70):
        g = plots.mosaic_geometry(B, *shape, max_size=48)
        assert (g['tile'], g['sf'], g['ns'], g['mosaic']) == (tile, sf, ns, (96, 68)) and 34 * 3 % 16 != 0
    images = _images(np.random.RandomState(B), B, *shape, kind)
    if kind != 'u8':
        _assert_specials_are_seen(images, n, ns, *tile, sf, *out)
    got, _ = run(images, n, ns, tile, sf, out)
    assert got.shape == (*out, 3)


# ------------------------------------------------------------------------------------------ predictions
def _boxes(rs, k, H, W):
    """Inside, wholly outside, across the tile's right / bottom edge (into the next tile or off the mosaic), across
    the top-left corner, degenerate, swapped; then random ones around the image."""
    box = [[W * .2, H * .3, W * .7, H * .8], [W + 300, H + 300, W + 320, H + 330], [-80, -90, -60, -70],
           [W * .6, H * .4, W * 1.3, H * .7], [W * .3, H * .6, W * .6, H * 1.4], [-5.5, -6.5, W * .3, H * .3],
           [W * .5, H * .2, W * .5, H * .9], [W * .8, H * .8, W * .2, H * .2], [W * .7, H * .7, W * 1.2, H * 1.2]]
    more = rs.rand(max(k - len(box), 0), 4) * [W + 40, H + 40, W + 40, H + 40] - 20
    return np.concatenate([np.array(box), more])[:k].astype(np.float32)


def _det(rs, B, max_det, H, W, nc):
    det = np.zeros((B, max_det, 6), np.float32)
    for b in range(B):
        det[b, :, :4] = _boxes(rs, max_det, H, W)
        det[b, :, 4] = rs.rand(max_det).astype(np.float32)
        det[b, :, 5] = rs.randint(0, nc + 2, max_det)       # some classes beyond the names
    return det


@pytest.mark.parametrize('shape, tile, sf', [((33, 65), (33, 65), 1.5), ((80, 112), (40, 56), 0.5),
                                             ((100, 70), (48, 34), 0.48)])
def test_gpu_mosaic_predictions(shape, tile, sf):
    """Counts 0, 1, max_det, negative and above max_det; conf at the threshold and its successor; a NaN and an inf
    row; classes -1, nc - 1, nc; boxes outside, across tile boundaries and across the mosaic's edge."""
    rs = np.random.RandomState(5)
    B, n, ns, max_det, nc = 6, 5, 3, 20, len(NAMES)
    det = _det(rs, B, max_det, shape[0], shape[1], nc)
    count = [0, 1, max_det, -3, max_det + 5, max_det]       # image 5 is no tile
    det[0, :, 4] = 0.9                                        # live-looking rows beyond count 0 and 1
    det[1, :, 4] = 0.9
    det[2, 0, 4] = 0.25
    det[2, 1, 4] = np.nextafter(np.float32(0.25), np.float32(1))
    det[2, 2, 4:] = [0.949999, 1]
    det[2, 3, 4:] = [0.95, 1]
    det[2, 4, 4:] = [1.0, 0]
    det[2, 5, 1] = np.nan
    det[2, 6, 2] = np.inf
    det[2, 7, 4:] = [0.8, -1]
    det[2, 8, 4:] = [0.8, nc]
    det[2, 9, 4:] = [0.8, nc - 1]
    det[2, 10, 4] = np.nan
    det[4, :, 4] = np.maximum(det[4, :, 4], np.float32(0.3))
    out = (ns * tile[0], ns * tile[1])
    got, _ = run(_images(rs, B, *shape, 'u8'), n, ns, tile, sf, out, det=det, count=count)
    rows = M.pred_rows(det, count, n, ns, *tile, sf)
    assert len(rows) >= 1 + 8 + max_det and not (rows[:, 4] == np.float32(0.25)).any()
    # and the downscale over the drawn boxes, without names
    run(_images(rs, B, *shape, 'f16'), n, ns, tile, sf, (out[0] * 2 // 3, out[1] // 2), det=det, count=count,
        names=None)


def test_gpu_mosaic_predictions_4800_rows():
    """max_det 300 with all 16 tiles full: more than one round of 256 records for every block of the pixel kernel."""
    rs = np.random.RandomState(6)
    B, max_det, shape = 16, 300, (40, 56)
    det = _det(rs, B, max_det, *shape, len(NAMES))
    det[:, :, 4] = np.float32(0.26) + det[:, :, 4] * np.float32(0.7)
    got, _ = run(_images(rs, B, *shape, 'u8'), 16, 4, shape, 2.0, (160, 224), det=det, count=[max_det] * B)
    assert len(M.pred_rows(det, [max_det] * B, 16, 4, *shape, 2.0)) == 4800


# ------------------------------------------------------------------------------------------ labels
@pytest.mark.parametrize('normalized', [True, False])
@pytest.mark.parametrize('shape, tile, sf', [((40, 56), (40, 56), 1.0), ((80, 112), (40, 56), 0.5)])
def test_gpu_mosaic_labels(normalized, shape, tile, sf):
    """Image 1 has no labels, images 4 and 5 are no tiles; a NaN row, classes -1 and nc."""
    rs = np.random.RandomState(8)
    B, n, ns, nc = 6, 4, 2, len(NAMES)
    per = [5, 0, 9, 3, 4, 2]
    L = sum(per)
    off = np.concatenate(([0], np.cumsum(per)))
    t = np.zeros((L, 6), np.float32)
    t[:, 0] = np.repeat(np.arange(B), per)
    t[:, 1] = rs.randint(0, nc + 1, L)
    t[:, 2:4] = rs.rand(L, 2) * 1.2 - 0.1
    t[:, 4:6] = rs.rand(L, 2) * 0.6
    if not normalized:
        t[:, 2:] *= [shape[1], shape[0], shape[1], shape[0]]
    t[6, 3] = np.nan
    t[7, 1] = -1
    t[8, 1] = nc
    rows = M.label_rows(t, off, n, ns, *tile, sf, normalized)
    assert len(rows) == 17
    run(_images(rs, B, *shape, 'f32'), n, ns, tile, sf, (ns * tile[0], ns * tile[1]), targets=t, label_off=off,
        normalized=normalized)


def test_gpu_mosaic_no_labels_at_all():
    rs = np.random.RandomState(9)
    images = _images(rs, 2, 33, 65, 'u8')
    got, _ = run(images, 2, 2, (33, 65), 1.0, (66, 130), targets=np.zeros((0, 6), np.float32), label_off=[0, 0, 0])
    bare, _ = run(images, 2, 2, (33, 65), 1.0, (66, 130))
    assert np.array_equal(got, bare)


# ------------------------------------------------------------------------------------------ captions
@pytest.mark.parametrize('shape, ns, n', [((40, 56), 2, 4), ((7, 5), 3, 5)])
def test_gpu_mosaic_captions(shape, ns, n):
    """Empty, 40 bytes (80 columns: over the next tile's caption and under its border, and in the last column past
    the mosaic's right edge), a byte >= 128; on 7 x 5 tiles the cells also reach below their tile."""
    rs = np.random.RandomState(10)
    long = b'forty bytes of caption, abc abc abc abc.'
    assert len(long) == 40
    captions = [long, b'', b'caf\xe9 abc', long, b'cab'][:n]
    out = (ns * shape[0], ns * shape[1])
    images = _images(rs, n, *shape, 'u8')
    got, _ = run(images, n, ns, shape, 2.0, out, captions=captions)
    bare, _ = run(images, n, ns, shape, 2.0, out, captions=[b''] * n)
    none, _ = run(images, n, ns, shape, 2.0, out)
    assert np.array_equal(bare, none) and not np.array_equal(got, bare)
    # with rows underneath and the downscale on top
    det = _det(rs, n, 6, *shape, len(NAMES))
    det[:, :, 4] = 0.5
    run(images, n, ns, shape, 2.0, (out[0] // 2, out[1] // 2) if shape[0] % 2 == 0 else (out[0] - 4, out[1] - 2),
        det=det, count=[6] * n, captions=captions)
