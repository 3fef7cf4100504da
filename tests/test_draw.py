"""plot_boxes (yv7_draw_boxes) against the numpy restatement of the contract (tests/draw_ref.py), torch.equal per
image, on random-noise images so that a stray or a missing write shows.  Tensor frames sit inside larger buffers
whose guard bytes are checked afterwards; numpy frames travel in one packed buffer, where a stray write lands in the
neighbouring frame.  Shapes are the smallest that can go wrong around the pixel kernel's TW x TH tile and its rounds
of 256 rows."""
import numpy as np
import pytest
import torch

import draw_ref as R
from utils import plots
from yv7 import _lib

pytestmark = pytest.mark.gpu

TW, TH = _lib.DRAW_TILE_W, _lib.DRAW_TILE_H
GUARD = 4096
PALETTE = [(200, 10, 20), (10, 220, 30), (20, 30, 240)]
NAMES = [b'a', b'abc', b'a name of thirty characters ..', b'caf\xe9', b'']
assert len(NAMES[2]) == 30


def _noise(rs, h, w):
    return rs.randint(0, 256, (h, w, 3)).astype(np.uint8)


def _special_boxes(h, w):
    """Inside, across each edge and each corner, fully outside, degenerate and swapped, with fractions."""
    return [[w * .25, h * .25, w * .75, h * .75], [-4.5, h * .3, w * .4, h * .6], [w * .6, h * .3, w + 5.5, h * .6],
            [w * .3, -6.2, w * .6, h * .4], [w * .3, h * .6, w * .6, h + 3.9], [-3, -3, w * .3, h * .3],
            [w * .7, -2, w + 2, h * .3], [-2, h * .7, w * .3, h + 2], [w * .7, h * .7, w + 4, h + 4],
            [w + 10, h + 10, w + 30, h + 30], [-50, 2, -20, 9], [w * .5, h * .2, w * .5, h * .8],
            [w * .4, h * .5, w * .4, h * .5], [w * .8, h * .8, w * .2, h * .2], [-0.9, -0.9, w - 0.1, h - 0.1],
            [-10, -10, w + 10, h + 10]]


def _rows(rs, h, w, n, nc):
    box = np.array(_special_boxes(h, w), np.float32)
    more = (rs.rand(max(n - len(box), 0), 4) * [w + 40, h + 40, w + 40, h + 40] - 20).astype(np.float32)
    box = np.concatenate([box, more])[:n]
    conf = rs.rand(n, 1).astype(np.float32)
    cls = rs.randint(0, nc + 2, (n, 1)).astype(np.float32)   # some classes beyond the names
    return np.concatenate([box, conf, cls], 1)


def _check(shapes, rows, counts, ts, max_det, names=None, atlas=None, reverse=False, tensor_frames=(), seed=0,
           palette=PALETTE):
    """rows[b]: [max_det, 6] (rows at and beyond count are live-looking boxes that must not be drawn)."""
    rs = np.random.RandomState(seed)
    B = len(shapes)
    originals = [_noise(rs, h, w) for h, w in shapes]
    frames, buffers = [], {}
    for b, im in enumerate(originals):
        if b in tensor_frames:
            buf = torch.from_numpy(rs.randint(0, 256, GUARD * 2 + im.size).astype(np.uint8)).cuda()
            buf[GUARD:GUARD + im.size] = torch.from_numpy(im.reshape(-1)).cuda()
            buffers[b] = buf, buf.cpu()
            frames.append(buf[GUARD:GUARD + im.size].view(im.shape))
        else:
            frames.append(im.copy())
    det = torch.from_numpy(np.stack(rows).astype(np.float32)).cuda()
    cnt = torch.tensor(counts, dtype=torch.int32).cuda()
    det0 = det.clone()
    dev_atlas = plots.Atlas(*atlas, det.device) if atlas is not None else None
    out = plots.plot_boxes(frames, det, cnt, names=names, colors=palette, line_thickness=list(ts), reverse=reverse,
                           atlas=dev_atlas)
    # read-only inputs (bitwise: a NaN row is not equal to itself)
    assert len(out) == B and torch.equal(det.view(torch.int32), det0.view(torch.int32)) and cnt.tolist() == list(counts)
    changed = 0
    for b, (im, t) in enumerate(zip(originals, ts)):
        n = min(max(counts[b], 0), max_det)
        host_atlas = atlas if atlas is not None else plots.glyph_atlas_host(plots.text_height(t))
        want = R.draw(im, rows[b][:n], palette, t, names=names, atlas=host_atlas if names is not None else None,
                      reverse=reverse)
        got = out[b].cpu().numpy()
        assert got.shape == want.shape
        if not np.array_equal(got, want):
            bad = np.argwhere((got != want).any(axis=2))
            raise AssertionError(f'image {b} {im.shape} t={t} count={counts[b]}: {len(bad)} pixels differ, first (y, x) '
                                 f'{bad[:5].tolist()} got {got[tuple(bad[0])]} want {want[tuple(bad[0])]}')
        changed += int((want != im).any())
        if b in tensor_frames:     # drawn in place, nothing outside the frame written
            assert out[b].data_ptr() == frames[b].data_ptr()
            buf, before = buffers[b]
            after = buf.cpu()
            assert torch.equal(after[:GUARD], before[:GUARD]) and torch.equal(after[-GUARD:], before[-GUARD:])
        else:                      # the caller's array is left alone
            assert np.array_equal(frames[b], im)
    return changed


SIZES = [(1, 1), (33, 51), (TH, TW), (TH + 1, TW + 1), (2 * TH + 3, 2 * TW + 5)]


@pytest.mark.parametrize('reverse', [False, True])
@pytest.mark.parametrize('labels', ['none', 'synthetic'])
def test_gpu_draw_sizes_counts_and_thickness(reverse, labels):
    """Five sizes around the tile, counts 0 / 1 / 17 / 300 and one beyond max_det (clamped), t = 1 .. 4, a NaN row
    and a negative class below count, numpy and tensor frames mixed."""
    assert SIZES[-1][1] % 2 == 1
    rs = np.random.RandomState(3)
    max_det = 300
    shapes = SIZES + [(33, 51), (TH + 1, TW + 1)]
    counts = [300, 17, 1, 0, 300, 305, -2]
    ts = [1, 2, 3, 4, 1, 4, 2]
    rows = [_rows(rs, h, w, max_det, len(NAMES)) for h, w in shapes]
    rows[1][5, 2] = np.nan
    rows[1][7, 5] = -1.0
    rows[4][100, 4] = np.inf
    rows[4][299, 0] = -np.inf
    names = NAMES if labels == 'synthetic' else None
    changed = _check(shapes, rows, counts, ts, max_det, names=names,
                     atlas=R.synthetic_atlas(4) if names else None, reverse=reverse, tensor_frames=(1, 3, 4), seed=4)
    assert changed >= 5     # every image with a positive count


@pytest.mark.parametrize('reverse', [False, True])
def test_gpu_draw_heavy_overlap_with_the_real_atlas(reverse):
    """40 boxes on one 64 x 64 region, names of 0, 1 and 30 characters, a non-ASCII byte, classes beyond the names,
    labels that run off the top and the right edge; the default atlases for t = 1 and t = 2."""
    rs = np.random.RandomState(7)
    shapes, max_det = [(100, 150), (2 * TH + 3, 2 * TW + 5)], 40
    rows = []
    for h, w in shapes:
        r = _rows(rs, h, w, max_det, len(NAMES))
        r[:, :4] = (rs.rand(max_det, 4) * 64 + [w - 70, 0, w - 70, 0]).astype(np.float32)   # top right region
        r[0, :4] = [w - 20, 3, w - 5, 30]      # label off the top and the right
        r[0, 5] = 2
        rows.append(r)
    assert _check(shapes, rows, [40, 40], [1, 2], max_det, names=NAMES, reverse=reverse, tensor_frames=(0,), seed=8) == 2


def test_gpu_draw_conf_ties_print_as_python_formats_them():
    """One label per tie on a grid, none overlapping: the digits the kernel draws are rint(conf * 100)'s."""
    ties = [0.125, 0.375, 0.625, 0.875]
    for v in [np.float32(0.005), np.float32(0.995)] + [np.float32(k / 200) for k in range(1, 200, 2)]:
        ties += [v, np.nextafter(v, np.float32(0)), np.nextafter(v, np.float32(1))]
    ties = np.array(ties, np.float32)
    n = len(ties)
    assert n == 4 + 3 * 102       # more than one round of 256 rows
    metrics, _ = plots.glyph_atlas_host(plots.text_height(1))
    cell_w = int(metrics[:, 1].max()) * 6 + 4
    per_row, pitch = 8, plots.text_height(1) + 8
    h, w = pitch * ((n + per_row - 1) // per_row) + 4, cell_w * per_row + 3
    rows = np.zeros((n, 6), np.float32)
    for i, c in enumerate(ties):
        x, y = (i % per_row) * cell_w + 1, (i // per_row + 1) * pitch
        rows[i] = [x, y, x + 2, y + 1, c, 0]
    assert _check([(h, w)], [rows], [n], [1], n, names=[b'x']) == 1
    # and the restatement's digits are Python's
    for c in ties:
        assert R.label_text(b'x', c) == f'x {float(c):.2f}'.encode()


@pytest.mark.parametrize('B', [1, 65])
def test_gpu_draw_batches_across_the_descriptor_chunk(B):
    rs = np.random.RandomState(B)
    shapes = [(20 + b % 7, 30 + b % 5) for b in range(B)]
    max_det = 7
    rows = [_rows(rs, h, w, max_det, len(NAMES)) for h, w in shapes]
    counts = [(b * 3) % 8 for b in range(B)] if B > 1 else [7]
    ts = [1 + b % 3 for b in range(B)]
    changed = _check(shapes, rows, counts, ts, max_det, names=NAMES, atlas=R.synthetic_atlas(5), reverse=bool(B % 2),
                     tensor_frames=tuple(range(0, B, 2)), seed=B + 1)
    assert changed == sum(c > 0 for c in counts)


def test_gpu_draw_default_thickness_and_palette():
    """line_thickness=None takes the reference's rule per frame, colors=None color_list()."""
    rs = np.random.RandomState(12)
    shapes = [(300, 330), (90, 70)]
    assert [plots.line_thickness(s) for s in shapes] == [2, 1]
    rows = [_rows(rs, h, w, 20, 3) for h, w in shapes]
    frames = [_noise(rs, h, w) for h, w in shapes]
    det, cnt = torch.from_numpy(np.stack(rows)).cuda(), torch.tensor([20, 20], dtype=torch.int32).cuda()
    names = ['person', 'bicycle', 'car']
    out = plots.plot_boxes(frames, det, cnt, names=names)
    for im, r, o in zip(frames, rows, out):
        t = plots.line_thickness(im.shape)
        want = R.draw(im, r, plots.color_list(), t, names=[n.encode() for n in names],
                      atlas=plots.glyph_atlas_host(plots.text_height(t)))
        assert np.array_equal(o.cpu().numpy(), want)
    assert plots.glyph_atlas(10) is plots.glyph_atlas(10)      # cached per (cell_h, device)


def test_gpu_draw_reads_nothing_back():
    """With the caches warm, plot_boxes on tensor frames enqueues its launches without a host synchronisation."""
    rs = np.random.RandomState(13)
    shapes = [(70, 90), (33, 51)]
    rows = [_rows(rs, h, w, 20, 3) for h, w in shapes]
    det, cnt = torch.from_numpy(np.stack(rows)).cuda(), torch.tensor([20, 7], dtype=torch.int32).cuda()
    names = ['person', 'bicycle', 'car']
    originals = [_noise(rs, h, w) for h, w in shapes]
    plots.plot_boxes([torch.from_numpy(f).cuda() for f in originals], det, cnt, names=names)     # warms the caches
    frames = [torch.from_numpy(f).cuda() for f in originals]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        with pytest.raises(RuntimeError):
            torch.ones(1, device='cuda').item()      # the mode must see a real sync, or it shows nothing
        out = plots.plot_boxes(frames, det, cnt, names=names)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    for im, r, n, o in zip(originals, rows, (20, 7), out):
        t = plots.line_thickness(im.shape)
        want = R.draw(im, r[:n], plots.color_list(), t, names=[s.encode() for s in names],
                      atlas=plots.glyph_atlas_host(plots.text_height(t)))
        assert np.array_equal(o.cpu().numpy(), want)
