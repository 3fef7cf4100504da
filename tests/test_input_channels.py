"""Model(cfg, ch=C) on the MI355X: the input packing kernel for any channel count (csrc/elementwise.hip input_kernel),
the unfused front end op by op, fp32 parity with the oracle, the fused stems for C = 1, 2, 4 (csrc/stem.hip:
stem2_kernel behind yolov7's stride-1 conv A, stem_kernel behind yolov7-tiny's stride-2 one, instantiated on
Planes<element type, C>), and the model API on such models.

Shapes: B = 2 (the image stride C * H * W is what a wrong channel count breaks), 64 x 96 — non-square; yolov7's stem
has 4 x 3 whole 8 x 16 output tiles there, yolov7-tiny's 2 x 2 with a partial 16-wide tile (its conv B output is 24
wide) — and 128 x 192 for yolov7-w6 (stride 64).  One case walks tiles persistently: yolov7, C = 1, B = 8 at
256 x 256 is 1024 stem tiles, above 256 CUs x 2 blocks.

Tolerances: the input packing is exact.  The unfused ops: tests/opcheck.py's (one fp16 ulp + 1e-4 rms; fp32 1e-5 + 1e-4
rms).  fp32 z: tests/parity.py against the oracle's fp32 and float64 forwards.  The fused stem: opcheck's STEM rule
restated for cin = C (stem_ref below: conv A's weights and bias pre-scaled by -log2 e and rounded to fp16 again where
both activations are SiLU, A rounded to fp16, conv B) with opcheck's own bars — at most 1e-3 of the elements beyond two
fp16 ulps + 1e-4 rms, max |d| <= 5e-3 rms; the bars were set for K = 27, the measured shares at K = 9 / 18 / 36 are in
DESIGN §4.24.  fp16 z end to end: rms-relative 0.05 against tests/family_ref.py, the bar of
tests/test_gpu_forward.py::test_forward_fp16_layerwise_scale.
"""
import copy
import functools

import pytest
import torch

import family_ref
from models.yolo import Model
from opcheck import _weights, check_ops, conv_ref, kernel_summary, rms_rel
from oracle import yolo_ref
from parity import check_z
from yv7 import _lib as L
from yv7.arch import get_cfg
from yv7.runtime import kernel_key
from yv7.synthetic import synthetic_frames, synthetic_state_dict

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
REFUSAL = 'this entry point loads 3-channel images; call the model on a \\[B,C,H,W\\] tensor'


@pytest.fixture(scope='module', autouse=True)
def _no_miopen():
    prev = torch.backends.cudnn.enabled
    torch.backends.cudnn.enabled = False
    yield
    torch.backends.cudnn.enabled = prev


@functools.lru_cache(maxsize=None)
def weights(name, C):
    """(cfg name, C) -> the state_dict of seeded synthetic weights (BatchNorm statistics from one 256 x 256 frame
    with C planes)."""
    m = Model(name, ch=C)
    return synthetic_state_dict(m, seed=0, calib_hw=256)


def fresh(name, C, fuse=True):
    m = Model(name, ch=C)
    m.load_state_dict(weights(name, C))
    m = m.float().eval()
    return m.fuse() if fuse else m


def planes(B, C, H, W, seed):
    return synthetic_frames(B, H, W, seed=seed, ch=C)


def reorg(x):   # ReOrg, models/common.py:52-53
    return torch.cat([x[..., ::2, ::2], x[..., 1::2, ::2], x[..., ::2, 1::2], x[..., 1::2, 1::2]], 1)


@functools.lru_cache(maxsize=None)
def oracle(name, C, B, H, W, seed):
    """x and the oracle's fp32 and float64 z for it, computed once."""
    net = yolo_ref.parse(get_cfg(name), ch_in=C)
    fused = yolo_ref.fuse(net, weights(name, C))
    x = planes(B, C, H, W, seed)
    return x, yolo_ref.forward(net, fused, x)[0], yolo_ref.forward64(net, fused, x)[0]


@functools.lru_cache(maxsize=None)
def family_z(name, C, B, H, W, seed):
    x = planes(B, C, H, W, seed)
    return x, family_ref.forward(fresh(name, C), x)[0]


def check_finite(plan, B, H, W):
    """Every op's output slice is finite (opcheck's |got - ref| > tol is false for a NaN, so it would pass):
    tests/test_family_gpu.py check_finite's rule."""
    for i, o in enumerate(plan.graph.ops):
        if o['kind'] in (L.OP_DETECT, L.OP_INPUT):
            continue
        c = o['cout2'] if o['kind'] == L.OP_STEM else o['cout']
        y = plan.tensor_view(o['dst'], B, H, W)[..., o['dst_coff']:o['dst_coff'] + c]
        assert torch.isfinite(y).all(), f'op {i} (kind {o["kind"]}): {int((~torch.isfinite(y)).sum())} outputs not finite'


# ------------------------------------------------------------------ 1. input packing, exact

@pytest.mark.parametrize('C', [1, 2, 4, 5, 8])
@pytest.mark.parametrize('name', ['yolov7-tiny', 'yolov7-w6'])
def test_input_packing_exact(name, C, monkeypatch):
    """The INPUT op's tensor: its first C (ReOrg: 4 C, group-major) channels are the image in the plan dtype, every
    padding channel is zero; fp32 and fp16 plans, fp32 and fp16 images.  (YV7_NO_STEM: the fp16 plans of C <= 4 would
    otherwise read the image in the fused stem.)"""
    monkeypatch.setenv('YV7_NO_STEM', '1')
    w6 = name == 'yolov7-w6'
    B, H, W = (2, 128, 192) if w6 else (2, 64, 96)
    torch.manual_seed(0)
    m = Model(name, ch=C).float().fuse().eval().to(DEV)   # (the packing does not depend on the weights)
    x32 = planes(B, C, H, W, seed=20 + C).to(DEV)
    for pdt in (torch.float32, torch.float16):
        plan = (m.half() if pdt == torch.float16 else m.float()).plan()
        o = plan.graph.ops[0]
        in_c = 4 * C if w6 else C
        assert (o['kind'], o['k'], o['cout']) == (L.OP_INPUT, 2 if w6 else 1, in_c) and plan.in_channels == C
        for xdt in (torch.float32, torch.float16):
            x = x32.to(xdt)
            kern = plan.op_kernels(B, H, W, xdt)[0]
            assert len(kern) == 1 and 'input_kernel' in kern[0], kern
            z = torch.empty((B, plan.num_rows(H, W), plan.no), dtype=torch.float32, device=DEV)
            plan.forward_into(x, z)
            torch.cuda.synchronize()
            t = plan.tensor_view(o['dst'], B, H, W)
            want = (reorg(x) if w6 else x).to(pdt).permute(0, 2, 3, 1)
            assert t.shape[-1] == plan.graph.tensors[o['dst']][0] >= in_c and t.shape[:3] == want.shape[:3]
            assert torch.equal(t[..., :in_c], want), (pdt, xdt)
            assert not t[..., in_c:].any(), (pdt, xdt)


# ------------------------------------------------------------------ 2. every op of the unfused path

@pytest.mark.parametrize('name,C,dtype', [('yolov7-tiny', 5, torch.float16), ('yolov7-tiny', 1, torch.float32),
                                          ('yolov7-w6', 1, torch.float32)], ids=['tiny-5-fp16', 'tiny-1-fp32', 'w6-1-fp32'])
def test_unfused_front_end_every_op(name, C, dtype):
    B, H, W = (2, 128, 192) if name == 'yolov7-w6' else (2, 64, 96)
    m = fresh(name, C).to(DEV)
    plan = (m.half() if dtype == torch.float16 else m).plan()
    assert plan.graph.ops[0]['kind'] == L.OP_INPUT and plan.graph.ops[1]['kind'] == L.OP_CONV
    x = planes(B, C, H, W, seed=7).to(DEV).to(dtype)
    z, xs = plan.forward(x)
    torch.cuda.synchronize()
    check_finite(plan, B, H, W)
    out = check_ops(plan, x, B, H, W, raw=xs, z=z)
    assert 0 in out and 1 in out and torch.isfinite(z).all()
    print(f'\n{name} C {C} {dtype}: {kernel_summary(out)}')


# ------------------------------------------------------------------ 3. fp32 parity

@pytest.mark.parametrize('C', [1, 4])
@pytest.mark.parametrize('name', ['yolov7-tiny', 'yolov7'])
def test_fp32_parity(name, C):
    B, H, W = 2, 64, 96
    x, z32, z64 = oracle(name, C, B, H, W, 3)
    m = fresh(name, C).to(DEV)
    z, _ = m(x.to(DEV))
    torch.cuda.synchronize()
    print('\n' + check_z(z, z32, z64, f'{name} C {C} fp32'))


# ------------------------------------------------------------------ 4. the fused stem

def stem_ref(plan, x):
    """The STEM op's output from the image, as tests/opcheck.py restates csrc/stem.hip's arithmetic, for cin = C:
    conv A's packed row is [32][9 C -> 64], k = tap * C + ci."""
    g = plan.graph
    o = g.ops[0]
    blob = g.weight_blob().to(plan.device)
    xin = x.half().float().permute(0, 2, 3, 1).contiguous()   # (the patch is fp16 whatever the image's dtype)
    wa, ba = _weights(plan, blob, o)
    wb, bb = _weights(plan, blob, dict(o, cin=o['cout'], cout=o['cout2'], w_off=o['w2_off'], b_off=o['b2_off']))
    if o['act'] == L.ACT_SILU and o['act2'] == L.ACT_SILU:
        nl2e = -1.4426950408889634
        za = conv_ref(xin, (wa * nl2e).half().float(), ba * nl2e, o['s'], L.ACT_NONE)
        a = (za / (1.0 + torch.exp2(za))).half().float()
        zb = conv_ref(a, wb, bb * nl2e, 2, L.ACT_NONE)
        return (zb * -0.6931471805599453) / (1.0 + torch.exp2(zb))
    a = conv_ref(xin, wa, ba, o['s'], o['act']).half().float()
    return conv_ref(a, wb, bb, 2, o['act2'])


def check_stem(plan, x, B, H, W, what):
    """opcheck's STEM bars; prints the measured shares before it asserts."""
    o = plan.graph.ops[0]
    got = plan.tensor_view(o['dst'], B, H, W)[..., o['dst_coff']:o['dst_coff'] + o['cout2']].float()
    ref = stem_ref(plan, x)
    assert got.shape == ref.shape and torch.isfinite(got).all(), what
    rms = ref.pow(2).mean().sqrt().item()
    d = (got - ref).abs()
    loose = int((d > torch.maximum(ref.abs(), got.abs()) * 2.0 ** -9 + 1e-4 * rms).sum())
    line = (f'{what}: K {9 * o["cin"]}, {loose} of {d.numel()} elements beyond two ulps (share {loose / d.numel():.3g}), '
            f'max |d| {d.max().item() / rms:.3g} rms')
    print('\n' + line)
    assert loose <= 1e-3 * d.numel(), line
    assert d.max().item() <= 5e-3 * rms, line
    return line


class _BehindTheStem:
    """The plan as tests/opcheck.py sees it without its STEM op (check_ops has no branch for an ADD and passes it by)."""

    def __init__(self, plan):
        self._plan = plan
        self.graph = copy.copy(plan.graph)
        self.graph.ops = [dict(o, kind=L.OP_ADD) if o['kind'] == L.OP_STEM else o for o in plan.graph.ops]

    def __getattr__(self, k):
        return getattr(self._plan, k)


STEM_KERNEL = {'yolov7': 'stem2_kernel', 'yolov7-tiny': 'stem_kernel'}


def is_stem_kernel(sym, kernel, xdt, C, sa):
    """sym, a name yv7_op_kernels reports, is `kernel` instantiated on Planes<element type, C> with conv A at stride sa
    (a name with _Float16 in it comes back mangled: the C++ runtime's demangler does not know the type)."""
    if xdt == torch.float16:
        return f'{len(kernel)}{kernel}INS0_6PlanesIDF16_Li{C}EEELi32ELi64ELi{sa}ELi8ELi16E' in sym
    return kernel_key(sym).startswith(f'{kernel}<Planes<float, {C}>, 32, 64, {sa}, 8, 16,')


@pytest.mark.parametrize('xdt', [torch.float16, torch.float32], ids=['x16', 'x32'])
@pytest.mark.parametrize('C', [1, 2, 4])
@pytest.mark.parametrize('name', ['yolov7', 'yolov7-tiny'])
def test_fused_stem(name, C, xdt):
    B, H, W = 2, 64, 96
    x, zref = family_z(name, C, B, H, W, 11)
    m = fresh(name, C).to(DEV).half()
    plan = m.plan()
    o = plan.graph.ops[0]
    assert o['kind'] == L.OP_STEM and o['cin'] == C and plan.in_channels == C
    kern = plan.op_kernels(B, H, W, xdt)[0]
    elem = '_Float16' if xdt == torch.float16 else 'float'
    assert len(kern) == 1 and is_stem_kernel(kern[0], STEM_KERNEL[name], xdt, C, o['s']), kern
    xg = x.to(DEV).to(xdt)
    z, xs = plan.forward(xg)
    torch.cuda.synchronize()
    check_stem(plan, xg, B, H, W, f'{name} C {C} {elem}')
    check_finite(plan, B, H, W)
    # the rest of the network behind it, op by op (check_ops' own STEM branch assumes 3 or 12 channels: skipped there)
    out = check_ops(_BehindTheStem(plan), xg, B, H, W, raw=xs, z=z)
    worst = rms_rel(z.cpu(), zref)
    print(f'{name} C {C} fp16: {kernel_summary(out)}; z rms-rel err {worst:.3g}')
    assert worst < 0.05


def test_three_channel_stem_keeps_its_kernel():
    """C = 3 launches the instantiation it always did (tests/golden/dispatch_fp16.txt pins the bench plans')."""
    for name, f16, f32 in (('yolov7', '_ZN3yv712_GLOBAL__N_112stem2_kernelIDF16_Li32ELi64ELi1ELi8ELi16ELi1ELi1EEEvNS_10StemParamsE',
                            'stem2_kernel<float, 32, 64, 1, 8, 16, 1, 1>'),
                           ('yolov7-tiny', '_ZN3yv712_GLOBAL__N_111stem_kernelIDF16_Li32ELi64ELi2ELi8ELi16ELi2ELi2EEEvNS_10StemParamsE',
                            'stem_kernel<float, 32, 64, 2, 8, 16, 2, 2>')):
        torch.manual_seed(0)
        plan = Model(name).float().fuse().eval().to(DEV).half().plan()
        assert plan.in_channels == 3
        assert plan.op_kernels(2, 64, 96)[0] == [f16]
        assert [kernel_key(k) for k in plan.op_kernels(2, 64, 96, torch.float32)[0]] == [f32]


def test_fused_stem_persistent_walk():
    """yolov7, C = 1, B = 8 at 256 x 256: 8 x 8 x 16 = 1024 stem tiles on at most 2 blocks per CU, so blocks walk on
    to second and later tiles (the prefetch of tile t + G under tile t, the deferred stores of tile t - G)."""
    name, C, B, H, W = 'yolov7', 1, 8, 256, 256
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tiles = B * ((H // 2 + 7) // 8) * ((W // 2 + 15) // 16)
    assert tiles == 1024 and tiles > 2 * cus
    plan = fresh(name, C).to(DEV).half().plan()
    x = planes(B, C, H, W, seed=13).to(DEV).half()
    z, _ = plan.forward(x)
    torch.cuda.synchronize()
    check_stem(plan, x, B, H, W, f'{name} C {C} B {B} {H}x{W}')
    assert torch.isfinite(z).all()


# ------------------------------------------------------------------ 5. the API

def test_augment_matches_the_oracle():
    name, C = 'yolov7-tiny', 1
    net = yolo_ref.parse(get_cfg(name), ch_in=C)
    fused = yolo_ref.fuse(net, weights(name, C))
    x = planes(2, C, 160, 224, seed=44)
    zr = yolo_ref.forward_augment(net, fused, x)
    z64 = yolo_ref.forward_augment(net, fused, x, f64=True)
    m = fresh(name, C).to(DEV)
    z, none = m(x.to(DEV), augment=True)
    torch.cuda.synchronize()
    assert none is None and z.shape == zr.shape
    print('\n' + check_z(z, zr, z64, f'{name} C {C} TTA'))


@pytest.mark.parametrize('half', [False, True], ids=['fp32', 'fp16'])
def test_wrong_channel_count_is_a_value_error(half):
    m = fresh('yolov7-tiny', 1).to(DEV)
    m = m.half() if half else m
    x = planes(2, 3, 64, 96, seed=1).to(DEV)
    with pytest.raises(ValueError, match=r'expected a \[B,1,H,W\] image batch .* got \(2, 3, 64, 96\)'):
        m(x.half() if half else x)
    plan = m.plan()
    z = torch.empty((2, plan.num_rows(64, 96), plan.no), dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError, match=r'\[B,1,H,W\]'):
        plan.forward_into(x, z)
    # and the other way round: a one-plane batch into a three-channel plan
    torch.manual_seed(0)
    m3 = Model('yolov7-tiny').float().fuse().eval().to(DEV)
    with pytest.raises(ValueError, match=r'expected a \[B,3,H,W\] image batch .* got \(2, 1, 64, 96\)'):
        m3(planes(2, 1, 64, 96, seed=1).to(DEV))


def test_ensemble_of_one_channel_models():
    from models.experimental import attempt_load
    a, b = fresh('yolov7-tiny', 1, fuse=False), fresh('yolov7-tiny', 1, fuse=False)
    ens = attempt_load([a, b], map_location=DEV)
    x = planes(2, 1, 64, 96, seed=5).to(DEV)
    z, _ = ens(x)
    z1, _ = fresh('yolov7-tiny', 1).to(DEV)(x)
    assert z.shape[1] == 2 * z1.shape[1] and torch.equal(z[:, :z1.shape[1]], z1) and torch.equal(z[:, z1.shape[1]:], z1)


def test_state_dict_checkpoint_with_ch_in_its_cfg(tmp_path):
    from models.experimental import attempt_load
    path = tmp_path / 'gray.pt'
    torch.save({'model': weights('yolov7-tiny', 1)}, path)
    cfg = get_cfg('yolov7-tiny')
    cfg['ch'] = 1
    m = attempt_load(str(path), map_location=DEV, cfg=cfg)
    assert m.yaml['ch'] == 1 and m.model[0].conv.in_channels == 1
    x = planes(2, 1, 64, 96, seed=9).to(DEV)
    z, _ = m(x)
    z0, _ = fresh('yolov7-tiny', 1).to(DEV)(x)
    torch.cuda.synchronize()
    assert torch.isfinite(z).all() and torch.equal(z, z0)


def test_entry_points_refuse_before_any_forward(tmp_path, monkeypatch):
    """detect.py's detect() and Model.autoshape() on a C = 1 model on the device: the documented RuntimeError, raised
    before the warm-up forward (a forward would raise the ValueError of the channel check instead)."""
    import yaml

    import detect
    from models.yolo import Model as M
    path, cfgp = tmp_path / 'gray.pt', tmp_path / 'gray.yaml'
    torch.save({'model': weights('yolov7-tiny', 1)}, path)
    cfg = get_cfg('yolov7-tiny')
    cfg['ch'] = 1
    cfgp.write_text(yaml.safe_dump(cfg))
    calls = []
    monkeypatch.setattr(M, 'forward', lambda self, *a, **k: calls.append(1))
    opt = detect.parse_opt(['--weights', str(path), '--cfg', str(cfgp), '--source', str(tmp_path), '--quiet'])
    with pytest.raises(RuntimeError, match=REFUSAL):
        detect.detect(opt)
    with pytest.raises(RuntimeError, match=REFUSAL):
        fresh('yolov7-tiny', 1).to(DEV).autoshape()
    assert not calls
