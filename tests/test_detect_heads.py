"""The Detect heads the benchmark runs — the call without raw logits: conv_det_rw_kernel (K = 256; K = 512
with 32-pixel tiles), conv_det_1tile_kernel, conv_det_pring_kernel (csrc/conv_det.hip launch_det_pring) and the
forced variant 94 — against a float64 reference of the same op, at the small shapes where they can break.

tests/opcheck.py's check_ops needs the raw logits, and a forward that returns them runs the 64 x 256 ring head
instead (det_pring_supported wants p.raw == nullptr).  Here every case calls forward_into(x, z, rowbest=rb) and
forward_into(x, z) (no records: the other counted waits of the heads' tile loops) and checks
  * Plan.op_kernels (a dry run without a raw pointer) names the expected head on every level — `expected_head`
    restates det_pring_supported / launch_det_pring, so a dispatch change cannot empty the test unnoticed;
  * z and rb are the inner B images of [B + 2, N, .] buffers filled with a NaN / a sentinel bit pattern: both
    guard images stay untouched bit for bit (the heads store through an unbounded buffer resource), no
    sentinel is left inside;
  * z against opcheck.check_detect_z: the float64 1x1 conv of the level's own input slice, decoded in float64
    (models/yolo.py:46-57), within the derived bound of opcheck.check_z_level;
  * z bit-equal to the z of plan.forward(x) — the raw path, which check_ops validates in the same case — and
    the z without records bit-equal to the z with them;
  * the row records exact: objectness, first-max class score and class from the z values themselves
    (utils/general.py:683-684).
Bit-equality of the two paths is something the code guarantees, not luck: every head and the ring kernel start
the accumulators at the bias, run the same 16 x 16 x 32 MFMA over K in ascending 32-channel steps, and share
det_sig and the decode's op order (conv_det.h), so it is asserted on every level.

Networks: three stride-2 convs to stride 8, then per level a 1x1 conv to the head's input width; level 0's
producer also feeds a Concat, so that head reads at a channel offset of a wider tensor.  Widths: every K a
shipped model gives a head — 128 / 256 / 512 (tiny), 256 / 512 / 1024 (yolov7), 768 (w6), 320 / 640 / 960 / 1280
(e6, e6e), 384 / 768 / 1152 / 1536 (d6).  det_pring_supported needs a level's first z row and the rows per image
to be multiples of 4, so with levels at strides 8 / 16 / 32 an odd stride-32 grid sends EVERY level to the ring
fallback, and a stride-8 level is then always whole tiles.  The `flat` layout (all three levels at stride 8)
lifts that: each head sees any grid with hw % 4 == 0.
"""
import copy
import functools

import pytest
import torch

from helpers import frames
from opcheck import check_detect_z, check_ops, kernel_summary
from yv7 import _lib as L
from yv7.runtime import kernel_key

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CUS = 256          # the MI355X; the per / grid figures in the comments below assume it
SENT = 0x7FA5A5A5  # the row records' sentinel: a NaN bit pattern no record holds
ANCHORS = [[12, 16, 19, 36, 40, 28], [36, 75, 76, 55, 72, 146], [142, 110, 192, 243, 459, 401]]
PYRAMID, FLAT = (8, 16, 32), (8, 8, 8)
WIDTHS = [(256, 512, 1024), (128, 768, 1280), (320, 640, 960), (384, 1152, 1536)]


@pytest.fixture(scope='module', autouse=True)
def _no_miopen():
    prev = torch.backends.cudnn.enabled
    torch.backends.cudnn.enabled = False
    yield
    torch.backends.cudnn.enabled = prev


def _c(f, c, k=1, s=1):
    return [f, 1, 'Conv', [c, k, s]]


def head_net(widths, strides):
    s0, s1, s2 = strides
    return {'nc': 80, 'depth_multiple': 1.0, 'width_multiple': 1.0, 'anchors': ANCHORS,
            'backbone': [_c(-1, 32, 3, 2), _c(-1, 64, 3, 2), _c(-1, 64, 3, 2),      # 0-2: stride 8
                         _c(2, widths[0]), _c(2, 64),                               # 3: level 0's input; 4
                         [[4, 3], 1, 'Concat', [1]],                                # 5: layer 3 at offset 64
                         _c(5, 64, 3, s1 // s0), _c(6, widths[1]),                  # 6; 7: level 1's input
                         _c(6, 64, 3, s2 // s1), _c(8, widths[2])],                 # 8; 9: level 2's input
            'head': [[[3, 7, 9], 1, 'Detect', ['nc', 'anchors']]]}


@functools.lru_cache(maxsize=None)
def head_plan(widths, strides):
    from models.yolo import Model
    from yv7.synthetic import synthetic_state_dict
    m = Model(copy.deepcopy(head_net(widths, strides)))
    m.load_state_dict(synthetic_state_dict(m, seed=3, calib_hw=256))
    m = m.float().eval().fuse().to(DEV).half()
    plan = m.plan()
    dets = sorted((o for o in plan.graph.ops if o['kind'] == L.OP_DETECT), key=lambda o: o['level'])
    assert [o['cin'] for o in dets] == list(widths) and plan.graph.stride == [float(s) for s in strides]
    assert (plan.na, plan.no) == (3, 85)
    assert dets[0]['src_coff'] > 0 and plan.graph.tensors[dets[0]['src']][0] > widths[0]   # a slice of the concat
    return m, plan


def expected_head(plan, o, B, H, W, row_off, nrows, variant):
    """(kernel key prefix, M, T, per, grid) of one DETECT op in the call without raw logits: det_pring_supported
    and launch_det_pring restated (csrc/conv_det.hip), with their tile counts."""
    s = int(plan.graph.stride[o['level']])
    hw, K = (H // s) * (W // s), o['cin']
    M = B * hw
    ok = (K % 64 == 0 and K >= 128 and hw % 4 == 0 and row_off % 4 == 0 and nrows % 4 == 0 and
          o['src_coff'] % 8 == 0 and plan.graph.tensors[o['src']][0] % 8 == 0)
    if not ok:   # the 64 x 256 ring (conv_f16.hip pick_det), two blocks per CU, one tile each
        return 'conv_f16_ring_kernel<64, 256,', M, (M + 63) // 64, 1, (M + 63) // 64
    bm = 32 if variant == 0 and K == 512 else 64
    T = (M + bm - 1) // bm
    per = (T + CUS - 1) // CUS
    grid = (T + per - 1) // per
    if variant == 0 and K == 256:
        return 'conv_det_rw_kernel<8, 0, 4, 64>', M, T, per, grid
    if variant == 0 and K == 512:
        return 'conv_det_rw_kernel<16, 0, 4, 32>', M, T, per, grid
    if variant == 0 and T <= CUS:
        return 'conv_det_1tile_kernel', M, T, 1, T
    return 'conv_det_pring_kernel<0>', M, T, per, grid


def run_case(widths, strides, B, H, W, variant=0):
    """One (net, B, H, W): the two calls without raw logits and the raw path; returns per level
    (kernel key, M, T, per, grid, worst ratio to check_z_level's bound)."""
    _, plan = head_plan(widths, strides)
    g = plan.graph
    dets = sorted(((i, o) for i, o in enumerate(g.ops) if o['kind'] == L.OP_DETECT), key=lambda t: t[1]['level'])
    x = frames(B, H, W, seed=17).to(DEV).half()
    N, no = plan.num_rows(H, W), plan.no
    for i, _ in dets if variant else []:
        plan.set_op_variant(i, variant)
    try:
        ks = plan.op_kernels(B, H, W)
        geo, row = [], 0
        for i, o in dets:
            want = expected_head(plan, o, B, H, W, row, N, variant)
            assert len(ks[i]) == 1 and kernel_key(ks[i][0]).startswith(want[0]), (o['level'], ks[i], want)
            geo.append((kernel_key(ks[i][0]),) + want[1:])
            s = int(g.stride[o['level']])
            row += plan.na * (H // s) * (W // s)
        assert row == N

        def call(records):
            zbuf = torch.full((B + 2, N, no), float('nan'), dtype=torch.float32, device=DEV)
            rbuf = torch.full((B + 2, N, 4), SENT, dtype=torch.int32, device=DEV)
            z, rb = zbuf[1:-1], rbuf[1:-1].view(torch.float32)
            assert z.is_contiguous() and rb.is_contiguous()
            plan.forward_into(x, z, rowbest=rb if records else None)
            torch.cuda.synchronize()
            for k in (0, -1):
                assert torch.isnan(zbuf[k]).all() and bool((zbuf[k].view(torch.int32) == 0x7FC00000).all()), \
                    f'z: guard image {k} written'
                assert bool((rbuf[k] == SENT).all()), f'row records: guard image {k} written'
            assert torch.isfinite(z).all(), f'{int((~torch.isfinite(z)).sum())} z elements not written / not finite'
            if records:
                assert bool((rbuf[1:-1] != SENT).all()), 'row records left at the sentinel'
            else:
                assert bool((rbuf == SENT).all()), 'row records written without a record buffer'
            return z, rb

        z1, rb = call(True)
        ratios = check_detect_z(plan, B, H, W, z1)
        z2, _ = call(False)
        check_detect_z(plan, B, H, W, z2)
        assert torch.equal(z1, z2), 'z differs between the calls with and without row records'
        obj = z1[..., 4]
        best, cls = (z1[..., 5:] * obj[..., None]).max(-1)
        assert torch.equal(rb[..., 0], obj) and torch.equal(rb[..., 1], best)
        assert torch.equal(rb[..., 2].view(torch.int32), cls.to(torch.int32))
        assert not rb[..., 3].any()
        # the raw path (the ring head), validated op by op, must give the same z bit for bit
        z0, xs = plan.forward(x)
        torch.cuda.synchronize()
        out = check_ops(plan, x, B, H, W, raw=xs, z=z0)
        row = 0
        for (i, o), gl in zip(dets, geo):
            n = gl[1] // B * plan.na
            assert torch.equal(z1[:, row:row + n], z0[:, row:row + n]), \
                f'level {o["level"]} ({gl[0]}): z differs from the raw path\'s z'
            row += n
    finally:
        for i, _ in dets if variant else []:
            plan.set_op_variant(i, 0)
    res = [gl + (ratios[o['level']][1],) for (i, o), gl in zip(dets, geo)]
    lay = 'flat' if strides == FLAT else 'pyramid'
    print(f'\n{lay} K {widths} B {B} {H}x{W}' + (f' variant {variant}' if variant else '') + ': ' + kernel_summary(out))
    for (i, o), (k, M, T, per, grid, r) in zip(dets, res):
        s = int(g.stride[o['level']])
        print(f'  level {o["level"]} K {o["cin"]} hw {(H // s) * (W // s)} M {M} T {T} per {per} grid {grid}: {k}, '
              f'worst z ratio to the bound {r:.3g}')
    return res


def kernels_of(res):
    return [r[0].split('<')[0] for r in res]


# Pyramid layout (levels at strides 8 / 16 / 32), 64-pixel tiles unless K = 512 (32):
#   B 5  64 x  64: hw 64 / 16 / 4, M 320 / 80 / 20   — a stride-32 tile spans all 5 images and is partial
#                  (20 of 64 rows); stride 16: T 2, each tile spans 4 images, the last holds 16 rows
#   B 5 128 x 128: hw 256 / 64 / 16, M 1280 / 320 / 80 — stride 32: T 2, 4 images per tile, last partial
#   B 1 128 x 384: hw 768 / 192 / 48, M = hw            — B = 1; stride 32: one partial tile of 48 rows
#   B 3 128 x 384: M 2304 / 576 / 144                    — stride 32: hw % 64 = 48, hw % 32 = 16, M % 64 = 16
#   B 3  96 x 160: hw 240 / 60 / 15                      — hw % 4 != 0 at stride 32: rows per image 945, so all
#                  three levels take the ring fallback
# Every persistent grid here is one tile per block (T <= 256 CUs).
PYRAMID_SHAPES = [(5, 64, 64), (5, 128, 128), (1, 128, 384), (3, 128, 384), (3, 96, 160)]


@pytest.mark.parametrize('B,H,W', PYRAMID_SHAPES)
@pytest.mark.parametrize('widths', WIDTHS)
def test_heads_pyramid(widths, B, H, W):
    res = run_case(widths, PYRAMID, B, H, W)
    if (H // 32) * (W // 32) % 4:
        assert all(k == 'conv_f16_ring_kernel' for k in kernels_of(res)), kernels_of(res)
    else:
        assert all(k.startswith('conv_det_') for k in kernels_of(res)), kernels_of(res)


# Flat layout (all levels at stride 8, so every K sees the same hw and M), small:
#   B 3  96 x 160: hw 12 x 20 = 240 (% 64 = 48, % 32 = 16), M 720: T 12 (last tile 16 rows) / 23 of 32 (last 16)
#   B 3  48 x  80: hw  6 x 10 =  60, M 180: T 3 (last 52) / 6 (last 20); every tile straddles images
#   B 3  80 x  80: hw 10 x 10 = 100, M 300: T 5 (last 44) / 10 (last 12)
#   B 3  32 x 160: hw  4 x 20 =  80 (% 64 = 16, % 32 = 16), M 240: T 4 (last 48) / 8 (last 16)
#   B 3  64 x  96: hw  8 x 12 =  96 (% 64 = 32), M 288: T 5 (last 32) / 9 whole
#   B 1  96 x 160: B = 1, M 240: T 4 (last 48) / 8 (last 16)
FLAT_SMALL = [(3, 96, 160), (3, 48, 80), (3, 80, 80), (3, 32, 160), (3, 64, 96), (1, 96, 160)]


@pytest.mark.parametrize('B,H,W', FLAT_SMALL)
@pytest.mark.parametrize('widths', WIDTHS)
def test_heads_flat_small(widths, B, H, W):
    res = run_case(widths, FLAT, B, H, W)
    want = ['conv_det_rw_kernel' if K in (256, 512) else 'conv_det_1tile_kernel' for K in widths]
    assert kernels_of(res) == want, kernels_of(res)   # K = 128: nk = 2, the one-tile ring's shortest loop


# Flat layout, more tiles than CUs (256), every level:
#   B 5 224 x 480: hw 28 x 60 = 1680 (% 64 = 16, % 32 = 16), M 8400 (% 64 = 16)
#       64-pixel tiles: T 132 <= 256 — the one-tile head at every K but 256 / 512; rw K 256: per 1, grid 132
#       32-pixel tiles (K 512): T 263, per 2, grid 132 (132 % 8 = 4: the plain walk), the last block has 1 tile
#   B 6 288 x 608: hw 36 x 76 = 2736 (% 64 = 48), M 16416 (% 64 = 32)
#       64: T 257 = CUs + 1, per 2, grid 129 (129 % 8 = 1), the last block has 1 tile — pring at every K but
#       256 / 512 (K 128: nk = 2, both prologue stages belong to one tile), rw at K 256
#       32 (K 512): T 513, per 3, grid 171
#   B 3 608 x 608: hw 76 x 76 = 5776 (% 64 = 16), M 17328 (% 64 = 48)
#       64: T 271, per 2, grid 136 = 8 x 17: the XCD-major walk with T % 8 = 7 — eighths of 33 / 34 tiles, so
#       the 17th block of an XCD has 1 or 2 tiles
#       32 (K 512): T 542, per 3, grid 181, the last block has 2 tiles
FLAT_LARGE = [(5, 224, 480), (6, 288, 608), (3, 608, 608)]


@pytest.mark.parametrize('B,H,W', FLAT_LARGE)
@pytest.mark.parametrize('widths', WIDTHS)
def test_heads_flat_more_tiles_than_cus(widths, B, H, W):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus != CUS:
        pytest.skip(f'the tile counts of these cases are chosen for {CUS} CUs (per >= 2, a short last block); '
                    f'this device has {cus}')
    res = run_case(widths, FLAT, B, H, W)
    for K, (k, M, T, per, grid, _) in zip(widths, res):
        if K == 256:
            assert k.startswith('conv_det_rw_kernel<8,')
        elif K == 512:
            assert k.startswith('conv_det_rw_kernel<16,') and per >= 2
        elif (B, H, W) == FLAT_LARGE[0]:
            assert k == 'conv_det_1tile_kernel' and T <= CUS
        else:
            assert k == 'conv_det_pring_kernel<0>' and per == 2 and T % per == 1
    if (B, H, W) == FLAT_LARGE[0]:   # the 32-pixel head's short last block on the plain walk
        assert [(T, per, grid) for K, (k, M, T, per, grid, _) in zip(widths, res) if K == 512] in ([], [(263, 2, 132)])
    if (B, H, W) == FLAT_LARGE[1]:
        assert all((T, per, grid) == (257, 2, 129) for K, (k, M, T, per, grid, _) in zip(widths, res) if K != 512)
    if (B, H, W) == FLAT_LARGE[2]:
        assert all((T, per, grid) == (271, 2, 136) for K, (k, M, T, per, grid, _) in zip(widths, res) if K != 512)


# Variant 94 — conv_det_pring_kernel with staged weights at every K, also 256 / 512 and where the one-tile head
# would run — forced on every level, through the calls without raw logits:
#   flat B 3 96 x 160 (M 720: T 12, image-straddling tiles, the last one 16 rows; one tile per block)
#   flat B 6 288 x 608 (T 257, per 2, grid 129: a short last block)
#   pyramid B 5 64 x 64 (M 320 / 80 / 20: one partial tile over 5 images)
@pytest.mark.parametrize('strides,B,H,W', [(FLAT, 3, 96, 160), (FLAT, 6, 288, 608), (PYRAMID, 5, 64, 64)])
@pytest.mark.parametrize('widths', WIDTHS[:2])
def test_variant_94_runs_the_persistent_head(widths, strides, B, H, W):
    if (B, H, W) == (6, 288, 608) and torch.cuda.get_device_properties(0).multi_processor_count != CUS:
        pytest.skip(f'T = 257 is one more than {CUS} CUs; this device has another count')
    res = run_case(widths, strides, B, H, W, variant=94)
    assert all(k == 'conv_det_pring_kernel<0>' for k, *_ in res), [r[0] for r in res]
