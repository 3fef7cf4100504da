"""The class-count-generic Detect head of fp16 plans (csrc/conv_det_nc.hip, conv_det_nc_kernel<NW>): every head
but the standard (na, no) = (3, 85), with and without raw logits, against a float64 reference of the same op.

Nets: tests/test_detect_heads.py's head_net (three levels, level 0 reading a channel slice of a concat) with the
class count and the anchors replaced.  Per case, in this order:
  1. BEFORE any launch, Plan.op_kernels (a dry run) names the kernel `expected_kernel` restates from the dispatch —
     conv_det_nc_kernel<width of no, ring slots> on every level of every small shape.  A tree without the kernel
     fails here, on the host: its 256-wide ring decodes one N tile only, so a head with
     na * no > 256 must never be launched there;
  2. z and the row records go into the inner B images of NaN / sentinel-filled [B + 2, N, .] buffers: the guard
     images stay untouched bit for bit, no sentinel is left inside;
  3. z against opcheck.check_detect_z (float64 conv + float64 decode) within check_z_level's derived bound; the
     worst ratio is printed;
  4. the row records exact from z: objectness, the FIRST maximum of z[..., 5:] * obj and its class (nc = 1:
     score == obj, class 0 — utils/general.py:669-670);
  5. plan.forward(x) (raw logits): check_ops passes and z is bit-equal to the z without raw logits;
  6. na * no <= 256 only: z bit-equal to the legacy 64 x 256 ring head (variant 99) on the same plan — both start
     the accumulators at the bias, run the same 16 x 16 x 32 MFMA over K in ascending 32-channel steps and share
     det_sig and the decode's op order (csrc/conv_det.h).

Class counts: 1, 3, 20, 79, 81, 83 and both ends of every compile-time width (32 / 64 / 96 / 144: nc 27 | 28,
59 | 60, 91 | 92, and 128, the largest the plan validation and the NMS admit), na = 3; one net each at na = 1, 2
and 4 (na = 4 at nc = 83: 352 channels).  K: (256, 512, 1024), and a net whose K are multiples of 8 but not of
64 (136, 200, 72: a zero-padded K tail of 8 in steps 3, 4 and 2).  Shapes (64-pixel tiles, one per block):
  B 5  64 x  64: hw 64 / 16 / 4 — a stride-32 tile is 20 of 64 rows over 5 images, a stride-16 tile spans 4
  B 3 128 x 384: hw 768 / 192 / 48, M 2304 / 576 / 144 — several blocks, partial last tiles
  B 3  96 x 160: hw 240 / 60 / 15 — hw % 4 != 0 at stride 32, rows per image 315 na: unaligned spans
  B 1  64 x  64: one image
and one flat-layout shape with more than 4 blocks per CU, where the dispatch takes its other paths
(test_nc_head_large_grid).
"""
import copy
import functools

import pytest
import torch

from helpers import frames
from opcheck import check_detect_z, check_ops, kernel_summary
from test_detect_heads import ANCHORS, DEV, FLAT, PYRAMID, SENT, WIDTHS, head_net, head_plan
from test_detect_heads import _no_miopen  # noqa: F401  (module-scoped autouse fixture)
from yv7 import _lib as L
from yv7.runtime import kernel_key

pytestmark = pytest.mark.gpu
NC_VARIANT = 89     # conv_det_nc_kernel forced on any DETECT op (csrc/conv_f16.hip pick_det)
RAGGED_K = (136, 200, 72)
SHAPES = [(5, 64, 64), (3, 128, 384), (3, 96, 160), (1, 64, 64)]


def anchors_of(na):
    """na anchors per level: the first na of the level's three, or a fourth between the last two."""
    out = []
    for lvl in ANCHORS:
        a = list(lvl) + [(lvl[2] + lvl[4]) // 2, (lvl[3] + lvl[5]) // 2]
        out.append(a[:2 * na])
    return out


def width_of(no):
    return next(w for w in (32, 64, 96, 144) if no <= w)


@functools.lru_cache(maxsize=None)
def nc_plan(nc, na=3, widths=WIDTHS[0], strides=PYRAMID, half=True):
    from models.yolo import Model
    from yv7.synthetic import synthetic_state_dict
    cfg = copy.deepcopy(head_net(widths, strides))
    cfg['nc'], cfg['anchors'] = nc, anchors_of(na)
    m = Model(cfg)
    m.load_state_dict(synthetic_state_dict(m, seed=3, calib_hw=256))
    m = m.float().eval().fuse().to(DEV)
    m = m.half() if half else m
    plan = m.plan()
    assert (plan.na, plan.no) == (na, nc + 5)
    dets = sorted(((i, o) for i, o in enumerate(plan.graph.ops) if o['kind'] == L.OP_DETECT), key=lambda t: t[1]['level'])
    assert [o['cin'] for _, o in dets] == list(widths) and all(o['cout'] == na * (nc + 5) for _, o in dets)
    return m, plan, dets


def buffers(plan, B, N):
    zbuf = torch.full((B + 2, N, plan.no), float('nan'), dtype=torch.float32, device=DEV)
    rbuf = torch.full((B + 2, N, 4), SENT, dtype=torch.int32, device=DEV)
    return zbuf, rbuf


def guarded_call(plan, x, B, N, records):
    """forward_into the inner images of guarded buffers -> (z, row records); the guards are checked."""
    zbuf, rbuf = buffers(plan, B, N)
    z, rb = zbuf[1:-1], rbuf[1:-1].view(torch.float32)
    assert z.is_contiguous() and rb.is_contiguous()
    plan.forward_into(x, z, rowbest=rb if records else None)
    torch.cuda.synchronize()
    for k in (0, -1):
        assert bool((zbuf[k].view(torch.int32) == 0x7FC00000).all()), f'z: guard image {k} written'
        assert bool((rbuf[k] == SENT).all()), f'row records: guard image {k} written'
    assert torch.isfinite(z).all(), f'{int((~torch.isfinite(z)).sum())} z elements not written / not finite'
    if records:
        assert bool((rbuf[1:-1] != SENT).all()), 'row records left at the sentinel'
    else:
        assert bool((rbuf == SENT).all()), 'row records written without a record buffer'
    return z, rb


def check_records(z, rb, nc):
    obj = z[..., 4]
    assert torch.equal(rb[..., 0], obj), 'row records: objectness'
    cls_got = rb[..., 2].view(torch.int32)
    if nc == 1:
        assert torch.equal(rb[..., 1], obj) and not cls_got.any(), 'row records: nc = 1 scores obj, class 0'
    else:
        sc = z[..., 5:] * obj[..., None]
        best = sc.max(-1).values
        idx = torch.arange(nc, device=z.device, dtype=torch.int32)
        first = torch.where(sc == best[..., None], idx, torch.full_like(idx, nc)).min(-1).values
        assert torch.equal(rb[..., 1], best), 'row records: best score'
        assert torch.equal(cls_got, first), 'row records: class of the first maximum'
    assert not rb[..., 3].any()


def expected_kernel(plan, o, B, H, W):
    """The kernel key of one DETECT op of a head other than (3, 85) under the tuned dispatch: pick_det
    (csrc/conv_f16.hip) and launch_det_nc (csrc/conv_det_nc.hip) restated."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    s = int(plan.graph.stride[o['level']])
    T = (B * (H // s) * (W // s) + 63) // 64
    cout = plan.na * plan.no
    if 240 < cout < 256 and T > cus:   # the ring's tile is more than 15/16 full, more than a tile per CU
        return 'conv_f16_ring_kernel<64, 256, 1, 4, 2, true, true>'
    w = width_of(plan.no)
    nblk = (T + 7) // 8 * 8 * plan.na
    return f'conv_det_nc_kernel<{w}, {3 if w <= 64 and nblk <= 4 * cus else 2}>'


def run_nc_case(nc, na, widths, B, H, W, strides=PYRAMID):
    _, plan, dets = nc_plan(nc, na, widths, strides)
    no = nc + 5
    ks = plan.op_kernels(B, H, W)   # step 1: nothing has been launched on this shape yet
    for i, o in dets:
        want = expected_kernel(plan, o, B, H, W)
        assert len(ks[i]) == 1 and kernel_key(ks[i][0]) == want, (o['level'], ks[i], want)
    x = frames(B, H, W, seed=17).to(DEV).half()
    N = plan.num_rows(H, W)
    z1, rb = guarded_call(plan, x, B, N, True)
    ratios = check_detect_z(plan, B, H, W, z1)
    z2, _ = guarded_call(plan, x, B, N, False)
    assert torch.equal(z1, z2), 'z differs between the calls with and without row records'
    check_records(z1, rb, nc)
    z0, xs = plan.forward(x)
    torch.cuda.synchronize()
    out = check_ops(plan, x, B, H, W, raw=xs, z=z0)
    assert all(tuple(r.shape[1:]) == (na, H // s, W // s, no) for r, s in zip(xs, (int(v) for v in plan.graph.stride)))
    assert torch.equal(z0, z1), 'z with raw logits differs from z without'
    if na * no <= 256:
        for i, _ in dets:
            plan.set_op_variant(i, 99)
        try:
            kr = plan.op_kernels(B, H, W)
            assert all(kernel_key(kr[i][0]).startswith('conv_f16_ring_kernel<64, 256,') for i, _ in dets), kr
            z9, _ = guarded_call(plan, x, B, N, False)
        finally:
            for i, _ in dets:
                plan.set_op_variant(i, 0)
        assert torch.equal(z9, z1), 'z differs from the 64 x 256 ring head (variant 99)'
    print(f'\nnc {nc} na {na} K {widths} B {B} {H}x{W}: {kernel_key(ks[dets[0][0]][0])}, {kernel_summary(out)}; worst z ratio to the bound per '
          f'level ' + ', '.join(f'{ratios[o["level"]][1]:.3g}' for _, o in dets))


NCS = [1, 3, 20, 27, 28, 59, 60, 79, 81, 83, 91, 92, 128]


@pytest.mark.parametrize('B,H,W', SHAPES)
@pytest.mark.parametrize('nc', NCS)
def test_nc_head(nc, B, H, W):
    run_nc_case(nc, 3, WIDTHS[0], B, H, W)


@pytest.mark.parametrize('B,H,W', SHAPES)
@pytest.mark.parametrize('nc,na', [(83, 1), (123, 2), (83, 4)])
def test_nc_head_other_anchor_counts(nc, na, B, H, W):
    run_nc_case(nc, na, WIDTHS[0], B, H, W)


@pytest.mark.parametrize('B,H,W', SHAPES)
@pytest.mark.parametrize('nc', [1, 20, 83])
def test_nc_head_ragged_k(nc, B, H, W):
    run_nc_case(nc, 3, RAGGED_K, B, H, W)


# Flat layout B 3 608 x 608: M 17328, T 271 on every level.  na 4: 1088 blocks > 4 per CU (256 CUs), so the narrow
# tiles run their two-slot ring (every shape above runs the three-slot one); nc 79 at na 3 (252 channels, T > CUs)
# stays on the 64 x 256 ring.
@pytest.mark.parametrize('nc,na', [(20, 4), (40, 4), (79, 3)])
def test_nc_head_large_grid(nc, na):
    B, H, W = 3, 608, 608
    _, plan, dets = nc_plan(nc, na, WIDTHS[0], FLAT)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus == 256:
        want = 'conv_f16_ring_kernel<64, 256,' if nc == 79 else f'conv_det_nc_kernel<{width_of(nc + 5)}, 2>'
        assert all(expected_kernel(plan, o, B, H, W).startswith(want) for _, o in dets)
    run_nc_case(nc, na, WIDTHS[0], B, H, W, FLAT)


@pytest.mark.parametrize('strides,B,H,W', [(PYRAMID, 5, 64, 64), (FLAT, 3, 96, 160)])
def test_forced_on_the_standard_head(strides, B, H, W):
    """Variant 89 on every level of the (3, 85) net: z bit-equal to the default heads' z, equal records."""
    _, plan = head_plan(WIDTHS[0], strides)
    dets = [i for i, o in enumerate(plan.graph.ops) if o['kind'] == L.OP_DETECT]
    x = frames(B, H, W, seed=17).to(DEV).half()
    N = plan.num_rows(H, W)
    k0 = plan.op_kernels(B, H, W)
    assert not any('conv_det_nc_kernel' in k0[i][0] for i in dets), k0   # the default dispatch of (3, 85) is not this
    z_def, rb_def = guarded_call(plan, x, B, N, True)
    for i in dets:
        plan.set_op_variant(i, NC_VARIANT)
    try:
        ks = plan.op_kernels(B, H, W)
        assert all(kernel_key(ks[i][0]).startswith('conv_det_nc_kernel<96, ') for i in dets), ks
        z, rb = guarded_call(plan, x, B, N, True)
        z_nr, _ = guarded_call(plan, x, B, N, False)
    finally:
        for i in dets:
            plan.set_op_variant(i, 0)
    assert torch.equal(z, z_def) and torch.equal(z_nr, z_def)
    assert torch.equal(rb.view(torch.int32), rb_def.view(torch.int32))
    check_records(z, rb, 80)


def test_legacy_det_forms_refuse_wide_heads():
    """nc = 83 (255 + 9 channels): the 256-wide forms cannot be forced; nothing is launched."""
    _, plan, dets = nc_plan(83)
    for i, _ in dets:
        for v in (92, 97, 99):
            with pytest.raises(RuntimeError, match='256'):
                plan.set_op_variant(i, v)
        assert plan.variants.get(i, 0) == 0


def test_fp32_plan_cross_check():
    """The fp32 plan of the nc = 83 net (the element-wise generic head of csrc/conv.hip) against the same
    float64 reference."""
    _, plan, dets = nc_plan(83, half=False)
    B, H, W = 3, 96, 160
    x = frames(B, H, W, seed=17).to(DEV)
    z, xs = plan.forward(x)
    torch.cuda.synchronize()
    ratios = check_detect_z(plan, B, H, W, z)
    check_ops(plan, x, B, H, W, raw=xs, z=z)
    print('\nfp32 nc 83: worst z ratio to the bound per level ' + ', '.join(f'{ratios[o["level"]][1]:.3g}' for _, o in dets))


@pytest.mark.parametrize('nc', [83, 1])
def test_end_to_end_custom_nc(nc):
    """Model('yolov7-tiny', nc=N), fp16, through the public call and the GPU NMS.

    z: every Detect level within check_z_level's bound of the float64 head on the plan's own inputs, and the
    whole z within the fp16 plans' bar against the fp32 oracle (rms-relative error < 0.05, the bar
    tests/test_gpu_forward.py holds every fp16 layer to).  NMS: bit-exact against oracle.nms_ref on the
    identical z, as tests/test_gpu_nms.py compares."""
    from models.yolo import Model
    from opcheck import rms_rel
    from oracle import nms_ref, yolo_ref
    from utils.general import non_max_suppression
    from yv7.synthetic import synthetic_state_dict
    m = Model('yolov7-tiny', nc=nc)
    assert m.yaml['nc'] == nc and len(m.names) == nc
    sd = synthetic_state_dict(m, seed=0)
    net = yolo_ref.parse(m.yaml)
    fused = yolo_ref.fuse(net, sd)
    B, H, W = 2, 128, 128
    x = frames(B, H, W, seed=6)
    zr, _ = yolo_ref.forward(net, fused, x)
    m.load_state_dict(sd)
    m = m.float().eval().fuse().to(DEV).half()
    plan = m.plan()
    ks = plan.op_kernels(B, H, W)
    want = f'conv_det_nc_kernel<{width_of(nc + 5)}, '
    assert all(kernel_key(ks[i][0]).startswith(want) for i, o in enumerate(plan.graph.ops) if o['kind'] == L.OP_DETECT), ks
    z = m(x.to(DEV).half())[0]
    torch.cuda.synchronize()
    assert tuple(z.shape) == tuple(zr.shape) and z.shape[-1] == nc + 5
    check_detect_z(plan, B, H, W, z.float())
    err = rms_rel(z.float().cpu(), zr)
    print(f'\nyolov7-tiny nc {nc} fp16: z rms-rel err vs the fp32 oracle {err:.3g}')
    assert err < 0.05
    zc = z.float().cpu()
    total = 0
    for kw in (dict(conf_thres=0.25, iou_thres=0.45), dict(conf_thres=0.001, iou_thres=0.65, multi_label=True)):
        out_r, rows_r = nms_ref.non_max_suppression(zc, return_rows=True, **kw)
        out_g, rows_g = non_max_suppression(z.float(), return_rows=True, **kw)
        for i in range(B):
            a, b = out_g[i].cpu(), out_r[i]
            assert a.shape == b.shape, (i, a.shape, b.shape)
            assert torch.equal(rows_g[i].cpu(), rows_r[i]), f'image {i}: kept rows differ'
            assert torch.equal(a, b), f'image {i}: detections differ'
            if nc > 1:
                assert bool((a[:, 5] < nc).all())
        n = sum(len(o) for o in out_r)
        assert n >= 1, f'no detection with {kw}'
        total += n
    print(f'  {total} detections')
