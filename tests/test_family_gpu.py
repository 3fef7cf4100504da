"""yolov7-e6 / -d6 / -e6e on the MI355X: the residual add kernel (csrc/elementwise.hip add_kernel, Shortcut
models/common.py:80-86), DownC's decomposition (common.py:181-192) and the three networks, op by op
(tests/opcheck.py, plus ADD here) and end to end against tests/family_ref.py.

Tolerances.  A conv with a residual: one fp16 ulp + 1e-4 rms of act(conv_ref) + res in fp32 on the op's own
inputs, opcheck's conv bar — the fused op rounds a correctly accumulated fp32 value once; against the unfused
conv + add two fp16 ulps (two roundings against one), the ulp taken at the larger of the sum and the conv output
the unfused pair rounds first (`_ulps`).  ADD: exact — fp16 + fp16 is exact in fp32, so the kernel's single rounding is torch's
(a.float() + b.float()).to(dtype).  fp32 plan z: tests/parity.py (1e-4 of scale + the reference's own distance
from float64, on every element).  fp16 plan: per layer and z, the rms-relative 0.05 of
tests/test_gpu_forward.py::test_forward_fp16_layerwise_scale.
"""
import copy

import pytest
import torch

import family_ref
from family_nets import fresh
from helpers import bordered, frames
from opcheck import _ulp_check, _weights, check_detect_z, check_ops, conv_ref, kernel_summary, rms_rel
from parity import check_z
from yv7 import _lib as L
from yv7.runtime import kernel_key

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module', autouse=True)
def _no_miopen():
    prev = torch.backends.cudnn.enabled
    torch.backends.cudnn.enabled = False
    yield
    torch.backends.cudnn.enabled = prev


def check_adds(plan, B, H, W):
    """Every ADD op of the last forward == torch's sum of its own operands, bit for bit."""
    n = 0
    dt = torch.float16 if plan.dtype == L.DT_F16 else torch.float32
    for i, o in enumerate(plan.graph.ops):
        if o['kind'] != L.OP_ADD:
            continue
        c = o['cout']
        a = plan.tensor_view(o['src'], B, H, W)[..., o['src_coff']:o['src_coff'] + c]
        b = plan.tensor_view(o['src2'], B, H, W)[..., o['src2_coff']:o['src2_coff'] + c]
        y = plan.tensor_view(o['dst'], B, H, W)[..., o['dst_coff']:o['dst_coff'] + c]
        assert torch.equal(y, (a.float() + b.float()).to(dt)), f'op {i} (ADD, {c} channels)'
        n += 1
    return n


def check_finite(plan, B, H, W):
    """Every op's output slice is finite (opcheck's |got - ref| > tol is false for a NaN, so it would pass)."""
    for i, o in enumerate(plan.graph.ops):
        if o['kind'] in (L.OP_DETECT, L.OP_INPUT):
            continue
        c = o['cout2'] if o['kind'] == L.OP_STEM else o['cout']
        y = plan.tensor_view(o['dst'], B, H, W)[..., o['dst_coff']:o['dst_coff'] + c]
        if not torch.isfinite(y).all():
            xin = plan.tensor_view(o['src'], B, H, W)[..., o['src_coff']:o['src_coff'] + o.get('cin', c)].float()
            raise AssertionError(f'op {i} (kind {o["kind"]}: {o.get("cin", 0)}->{c} k{o.get("k", 1)} s{o.get("s", 1)}): '
                                 f'{int((~torch.isfinite(y)).sum())} of {y.numel()} outputs not finite; its input: '
                                 f'max |x| {xin.abs().max().item():.4g}, finite {bool(torch.isfinite(xin).all())}')


def is_res(o):
    return o['kind'] == L.OP_CONV and o.get('src2', -1) >= 0


def check_residuals(plan, B, H, W, only=None):
    """Every conv that carries a residual: act(conv_ref(x)) + res in fp32 on the op's own inputs, opcheck's conv
    bar (one fp16 ulp + 1e-4 rms).  Returns {op: worst rel err}."""
    blob = plan.graph.weight_blob().to(plan.device)
    out = {}
    for i, o in enumerate(plan.graph.ops):
        if not is_res(o) or (only is not None and i != only):
            continue
        c = o['cout']
        xin = plan.tensor_view(o['src'], B, H, W)[..., o['src_coff']:o['src_coff'] + o['cin']].float()
        w, b = _weights(plan, blob, o)
        res = plan.tensor_view(o['src2'], B, H, W)[..., o['src2_coff']:o['src2_coff'] + c].float()
        ref = conv_ref(xin, w, b, o['s'], o['act']) + res
        got = plan.tensor_view(o['dst'], B, H, W)[..., o['dst_coff']:o['dst_coff'] + c]
        out[i] = _ulp_check(got, ref, f'op {i} (CONV + residual: {o["cin"]}->{c} k{o["k"]} s{o["s"]})', True)
    return out


class _NoResidual:
    """The plan as tests/opcheck.py sees it: opcheck knows no residual, so those convs are left to check_residuals."""

    def __init__(self, plan):
        self._plan = plan
        self.graph = copy.copy(plan.graph)
        self.graph.ops = [dict(o, kind=L.OP_ADD) if is_res(o) else o for o in plan.graph.ops]

    def __getattr__(self, k):
        return getattr(self._plan, k)


def check_all(plan, x, B, H, W, z, xs):
    check_finite(plan, B, H, W)
    out = check_ops(_NoResidual(plan), x, B, H, W, raw=xs, z=z)
    out.update(check_residuals(plan, B, H, W))
    kinds = {o['kind'] for o in plan.graph.ops}
    assert kinds <= {L.OP_INPUT, L.OP_CONV, L.OP_MAXPOOL, L.OP_UPSAMPLE, L.OP_DETECT, L.OP_ADD}, kinds   # all checked
    return out, check_adds(plan, B, H, W)


def check_no_raw_call(plan, x, B, H, W, z_raw):
    """The call without raw logits (the benchmark's): it alone runs the persistent Detect heads (csrc/conv_det.hip;
    a forward that returns raw logits runs the 64 x 256 ring), so check_ops above never sees them.  z into a
    NaN-filled buffer with a guard image on either side, against the float64 reference that needs no raw logits
    (opcheck.check_detect_z), and bit-equal to the raw path's z (the heads promise the ring kernel's arithmetic).
    Returns a line naming each level's head kernel and its worst ratio to the bound."""
    N = plan.num_rows(H, W)
    zbuf = torch.full((B + 2, N, plan.no), float('nan'), dtype=torch.float32, device=x.device)
    z = zbuf[1:-1]
    plan.forward_into(x, z)
    torch.cuda.synchronize()
    assert torch.isnan(zbuf[0]).all() and torch.isnan(zbuf[-1]).all(), 'z written outside its images'
    ratios = check_detect_z(plan, B, H, W, z)
    assert torch.equal(z, z_raw), 'z without raw logits differs from the raw path\'s z'
    ks = plan.op_kernels(B, H, W)
    return 'without raw logits: ' + ', '.join(f'K {plan.graph.ops[i]["cin"]} {kernel_key(ks[i][0])} {r:.3g}'
                                              for _, (i, r) in sorted(ratios.items()))


@pytest.mark.parametrize('c', [8, 160])
@pytest.mark.parametrize('dtype', [torch.float16, torch.float32], ids=['fp16', 'fp32'])
def test_add_kernel_exact_in_concat_slices(dtype, c):
    """Both operands and the sum at non-zero channel offsets of wider tensors (three different pitches), one
    16-byte vector (c = 8) and 160 channels, B = 3 at 96 x 160 (the add runs at 12 x 20): exact, and the
    zero frames of all three tensors intact."""
    B, H, W = 3, 96, 160
    m = fresh(('add', c)).to(DEV)
    m = m.half() if dtype == torch.float16 else m
    plan = m.plan()
    adds = [o for o in plan.graph.ops if o['kind'] == L.OP_ADD]
    assert len(adds) == 1
    o = adds[0]
    pitches = [plan.graph.tensors[o[k]][0] for k in ('src', 'src2', 'dst')]
    assert o['src_coff'] > 0 and o['src2_coff'] > 0 and o['dst_coff'] > 0 and min(pitches) > c and o['cout'] == c
    assert len({o['src'], o['src2'], o['dst']}) == 3
    x = frames(B, H, W, seed=21).to(DEV).to(dtype)
    plan.forward(x)
    torch.cuda.synchronize()
    assert check_adds(plan, B, H, W) == 1
    for k in ('src', 'src2', 'dst'):
        t = bordered(plan, o[k], B, H, W)
        assert t.shape[1:3] == (H // 8 + 2, W // 8 + 2)
        frame = t.clone()
        frame[:, 1:-1, 1:-1] = 0
        assert not frame.any(), f'{k}: zero frame overwritten'
        assert t[:, 1:-1, 1:-1].float().abs().sum() > 0
    kern = plan.op_kernels(B, H, W, dtype)[plan.graph.ops.index(o)]
    assert len(kern) == 1 and 'add_kernel' in kern[0], kern


def _ulps(a, b, mid):
    """|a - b| in fp16 ulps (normal range), the ulp taken at the largest of |a|, |b| and |mid|.  a: the fused
    conv + residual, one rounding of the fp32 sum; b: the unfused pair, which first rounds the conv output `mid`
    (half an ulp of |mid|) and then the sum (half an ulp of |b|).  Where conv output and residual cancel, the
    first rounding is many ulps of the small sum, so the two-ulp bound is stated at the operands' magnitude."""
    a, b = a.float(), b.float()
    mx = torch.maximum(torch.maximum(a.abs(), b.abs()), mid.float().abs()).clamp(min=2.0 ** -14)
    return ((a - b).abs() / 2.0 ** (torch.floor(torch.log2(mx)) - 10)).max().item()


# variant -> the kernel it must launch on a conv with a residual: the register-staged tile kernel (1), the 8-wave
# ring (4: 256 x 128, 6: 128 x 128, 110: 256 x 128 by the ring rule) and its split-K hand-off (132 / 134: the
# 128 x 128 ring with 2 / 4 K parts, 142: 128 x 64 with 2), and the tuned choice (0)
RES_VARIANTS = {0: 'res_kernel', 1: 'conv_f16_res_kernel', 4: 'conv_f16_ring_res_kernel', 6: 'conv_f16_ring_res_kernel',
                110: 'conv_f16_ring_res_kernel', 132: 'conv_f16_ring_res_kernel', 134: 'conv_f16_ring_res_kernel',
                142: 'conv_f16_ring_res_kernel'}


@pytest.mark.parametrize('kin', [320, 80])
def test_fused_residual_every_kernel(kin, monkeypatch):
    """A Shortcut folded into its 1x1 conv, forced onto each kernel that has the residual epilogue and onto the
    ring's split-K reduce: cout 160 (the last N tile masked), M = 3 x 12 x 20 = 720 (no multiple of a tile
    height), K = 320 and the ragged K = 80, residual pitch 320 at offset 160, destination pitch 192 at offset 32."""
    B, H, W = 3, 96, 160
    monkeypatch.delenv('YV7_RESFUSE', raising=False)
    monkeypatch.setenv('YV7_NO_RESFUSE', '1')
    base = fresh(('res', kin)).to(DEV).half().plan()
    monkeypatch.delenv('YV7_NO_RESFUSE')
    monkeypatch.setenv('YV7_RESFUSE', '1')
    plan = fresh(('res', kin)).to(DEV).half().plan()
    assert sum(o['kind'] == L.OP_ADD for o in base.graph.ops) == 1 and not any(is_res(o) for o in base.graph.ops)
    ri = [i for i, o in enumerate(plan.graph.ops) if is_res(o)]
    assert len(ri) == 1 and not any(o['kind'] == L.OP_ADD for o in plan.graph.ops)
    i, o = ri[0], plan.graph.ops[ri[0]]
    assert (o['cin'], o['cout'], o['k']) == (kin, 160, 1)
    assert plan.graph.tensors[o['src2']][0] == 320 and o['src2_coff'] == 160
    assert plan.graph.tensors[o['dst']][0] == 192 and o['dst_coff'] == 32
    x = frames(B, H, W, seed=13).to(DEV).half()
    base.forward(x)
    torch.cuda.synchronize()
    t8, off8, c8 = base.graph.layer_tensor[8]
    unfused = base.tensor_view(t8, B, H, W)[..., off8:off8 + c8].clone()
    t7, off7, c7 = base.graph.layer_tensor[7]
    conv7 = base.tensor_view(t7, B, H, W)[..., off7:off7 + c7].clone()   # the unfused conv's rounded output
    dst0 = bordered(base, t8, B, H, W).clone()
    res0 = bordered(base, base.graph.layer_tensor[4][0], B, H, W).clone()
    with pytest.raises(RuntimeError, match='residual'):
        plan.set_op_variant(i, 201)   # the persistent ring has no residual epilogue
    lines = []
    for v, kernel in RES_VARIANTS.items():
        plan.set_op_variant(i, v)
        kern = plan.op_kernels(B, H, W)[i]
        assert len(kern) == 1 and kernel in kern[0], (v, kern)
        plan.forward(x)
        torch.cuda.synchronize()
        worst = check_residuals(plan, B, H, W, only=i)[i]
        got = plan.tensor_view(o['dst'], B, H, W)[..., o['dst_coff']:o['dst_coff'] + 160]
        assert torch.isfinite(got).all()
        u = _ulps(got, unfused, conv7)
        assert u <= 2.0, f'variant {v}: fused vs conv + add differ by {u} fp16 ulps'
        # outside the written slice the destination tensor is what the unfused plan has there (layer 9's output
        # and the zero frame), and the residual's tensor is untouched: byte for byte
        dst = bordered(plan, o['dst'], B, H, W)
        keep = torch.ones(192, dtype=torch.bool, device=dst.device)
        keep[32:192] = False
        assert torch.equal(dst[..., keep].view(torch.int16), dst0[..., keep].view(torch.int16)), v
        frame = dst.clone()
        frame[:, 1:-1, 1:-1] = 0
        assert not frame.any(), f'variant {v}: zero frame overwritten'
        assert torch.equal(bordered(plan, o['src2'], B, H, W).view(torch.int16), res0.view(torch.int16)), v
        lines.append(f'variant {v} ({kernel_key(kern[0])}): worst rel {worst:.3g}, {u:.2f} ulps from conv + add')
    print('\n' + '\n'.join(lines))


@pytest.fixture(scope='module')
def mini_refs():
    m = fresh(('mini',))
    x = frames(2, 128, 128, seed=5)
    (z32, _), outs = family_ref.forward(m, x, return_all=True)
    z64, _ = family_ref.forward(m, x, torch.float64)
    return x, z32, z64, outs


def test_mini_e6e_fp32(mini_refs):
    x, z32, z64, _ = mini_refs
    B, H, W = 2, 128, 128
    m = fresh(('mini',)).to(DEV)
    plan = m.plan()
    xg = x.to(DEV)
    z, xs = plan.forward(xg)
    torch.cuda.synchronize()
    out, n = check_all(plan, xg, B, H, W, z, xs)
    assert n == 2
    print('\nmini-e6e fp32: ' + kernel_summary(out) + '; ' + check_z(z, z32, z64, 'mini-e6e fp32'))


@pytest.mark.parametrize('fuse', ['add', 'residual'])
def test_mini_e6e_fp16(mini_refs, fuse, monkeypatch):
    x, z32, _, outs = mini_refs
    B, H, W = 2, 128, 128
    monkeypatch.delenv('YV7_RESFUSE', raising=False)
    monkeypatch.delenv('YV7_NO_RESFUSE', raising=False)
    monkeypatch.setenv('YV7_NO_RESFUSE' if fuse == 'add' else 'YV7_RESFUSE', '1')
    m = fresh(('mini',)).to(DEV).half()
    plan = m.plan()
    xg = x.to(DEV).half()
    z, xs = plan.forward(xg)
    torch.cuda.synchronize()
    out, n = check_all(plan, xg, B, H, W, z, xs)
    assert n + sum(is_res(o) for o in plan.graph.ops) == 2 and n == (2 if fuse == 'add' else 0)
    worst = rms_rel(z.cpu(), z32)
    for i in sorted(plan.graph.layer_tensor):
        if isinstance(outs[i], torch.Tensor):
            worst = max(worst, rms_rel(plan.layer_output(i, B, H, W).cpu(), outs[i]))
    print(f'\nmini-e6e fp16: {kernel_summary(out)}; worst rms-rel err {worst:.3g}')
    assert worst < 0.05
    print(check_no_raw_call(plan, xg, B, H, W, z))


@pytest.mark.parametrize('name,fuse', [('yolov7-e6', 'default'), ('yolov7-d6', 'default'), ('yolov7-e6e', 'default'),
                                       ('yolov7-e6e', 'residual')])
def test_full_model_fp16_every_op(name, fuse, monkeypatch):
    """The tuned dispatch on widths no earlier model has (cin 12 / 80 / 96 / 160 / 192 / 480 / 576 / 960 / 1152,
    cout up to 1536): every op of a B = 2, 128 x 128 forward against its fp32 reference; e6e also with every
    Shortcut folded into its conv (YV7_RESFUSE=1)."""
    B, H, W = 2, 128, 128
    monkeypatch.delenv('YV7_RESFUSE', raising=False)
    monkeypatch.delenv('YV7_NO_RESFUSE', raising=False)
    if fuse == 'residual':
        monkeypatch.setenv('YV7_RESFUSE', '1')
    # (weights calibrated at 256 x 256: at 128 the stride-64 level has four pixels per channel, too few for
    # BatchNorm statistics — such weights push the activations of other frames past the fp16 range)
    m = fresh(name, calib_hw=256).to(DEV).half()
    plan = m.plan()
    x = frames(B, H, W, seed=9).to(DEV).half()
    z, xs = plan.forward(x)
    torch.cuda.synchronize()
    out, n = check_all(plan, x, B, H, W, z, xs)
    nres = sum(is_res(o) for o in plan.graph.ops)
    assert n + nres == (11 if name == 'yolov7-e6e' else 0) and (fuse != 'residual' or nres == 11)
    assert torch.isfinite(z).all()
    print(f'\n{name} fp16 ({fuse}): {kernel_summary(out)}, {n} adds exact, {nres} residual convs')
    # the head widths of these models (320 / 640 / 960 / 1280, d6: 384 / 768 / 1152 / 1536) in their own graphs:
    # at this size every level is a single tile, so the one-tile head runs its 5 to 24 K steps
    line = check_no_raw_call(plan, x, B, H, W, z)
    print(line)
    assert line.count('conv_det_1tile_kernel') == 4, line


def test_model_api_end_to_end(tmp_path):
    """attempt_load of a pickled DownC / Shortcut model -> model(img)[0] -> non_max_suppression; a CPU tensor
    still raises."""
    from models.experimental import attempt_load
    from utils.general import non_max_suppression
    src = fresh(('mini',), fuse=False).half()
    del src._plans
    path = tmp_path / 'mini-e6e.pt'
    torch.save({'model': src, 'ema': None}, path)
    model = attempt_load(str(path), map_location=DEV)
    x = frames(2, 128, 128, seed=5)
    with pytest.raises(RuntimeError, match='ROCm'):
        model(x)
    pred = model(x.to(DEV))[0]
    torch.cuda.synchronize()
    m16 = fresh(('mini',), fuse=False).half().float().fuse()   # the checkpoint's fp16-rounded weights
    z32, _ = family_ref.forward(m16, x)
    z64, _ = family_ref.forward(m16, x, torch.float64)
    check_z(pred, z32, z64, 'mini-e6e via attempt_load')
    det = non_max_suppression(pred, 0.25, 0.45)
    assert len(det) == 2 and all(d.shape[1] == 6 for d in det)
