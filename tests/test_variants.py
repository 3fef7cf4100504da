"""Every kernel configuration of the fp16 conv dispatch, forced onto every conv op of a real network
(yv7_set_op_variant), checked op by op against a plain PyTorch fp32 reference of the same op on the
op's own input (tests/opcheck.py).

The tuned dispatch (csrc/conv_f16.hip pick_tuned / choose; the forced variants are its forced_rows table,
the launch tables csrc/conv_f16_launch.h) picks among these by tile count, so
a small frame exercises only some of them; forcing each one on every layer shape of yolov7 /
yolov7-tiny covers them all: the generic tile kernels (1, 2, 8), the 8-wave LDS-DMA rings (4-7),
the halo and weight-stationary 3x3 kernels (10, 11, and 15: its half-patch ring form), every ring configuration with 1, 2 and 4 K
splits (1CS: configuration C, S splits; the split-K hand-off of splitk_reduce), the persistent rings
(201-206), the 8-phase rings (231: 256 x 256, 232: 256 x 128), the weight-stationary 1x1 rings (234-236,
and 239: N-split), the column-group 3x3 halo ring (262), the
low-resolution 3x3 kernel (270-273: 80 / 64-pixel tiles of 4 images x 4 columns, 128 / 64 channels;
274 / 277-279: stride 2; 275 / 276: 160-pixel tiles), the register-weight 3x3 kernel (280-284: stride 2,
285-288: stride 1; cin 64 / 128, 2-5 ring slots, 2-8-row tiles, with and without the stagger), the register-weight 1x1 kernel (290-295: cin 128 / 256 / 512, with and
without the stagger; 302 / 303: cin 256 with 128-channel N slices) and
the alternative Detect heads (92, 97, and 99: the 64 x 256 ring that was the default before the
persistent head; 94: the persistent head with staged weights).  A forward that returns raw logits never runs
a persistent head (det_pring_supported admits it only without them: 94 then runs the 64 x 256 ring), so the
Detect variants also run through the call without raw logits, where 94 must launch conv_det_pring_kernel;
that z is checked against a float64 reference and against the raw path's z (_check_no_raw_call; the default
heads at their awkward shapes: tests/test_detect_heads.py).  A variant a layer's shape
does not support runs the register-staged tile kernel instead (conv_f16.hip pick_forced), which the check
then covers again; test_every_conv_variant prints, per variant, the ops on which another kernel than that fallback
launched, and test_variants_that_launch_nowhere pins the variants that only ever fall back on both networks
(tests/test_gemm_edges.py and tests/test_addr_trim.py hold every variant to its own kernel on nets built for it).
Reference computation: models/common.py:110-111 (Conv.fuseforward), models/yolo.py:46-57 (Detect).
"""
import pytest
import torch

from helpers import fresh_model, frames
from opcheck import check_detect_z, check_ops, kernel_summary
from yv7 import _lib as L
from yv7.runtime import kernel_key

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

CONV_VARIANTS = [1, 2, 4, 5, 6, 7, 8, 10, 11, 15, 17,
                 100, 102, 104, 110, 112, 114, 120, 122, 124, 130, 132, 134, 140, 142, 144, 150, 152, 154,
                 201, 202, 203, 204, 205, 206, 231, 232, 234, 235, 236, 239, 262, 270, 271, 272, 273, 274, 275, 276,
                 277, 278, 279, 280, 281, 282, 283, 284, 285, 286, 287, 288, 290, 291, 292, 293,
                 294, 295, 302, 303]
DET_VARIANTS = [92, 94, 97, 99]
NETWORKS = [('yolov7', 2, 256, 256), ('yolov7-tiny', 2, 192, 256)]
# The forced variants that launch nothing but the fallback on every conv op of both networks at these frames: today's
# silent fallbacks, pinned so that a dispatch change which adds one shows up.  (Six configurations of conv_lr.hip whose
# tile heights divide no map of these frames; tests/test_addr_trim.py launches them.)
LAUNCH_NOWHERE = [270, 271, 275, 276, 277, 279]
LAUNCHED = {}   # network -> {variant: [ops on which a kernel other than the fallback launched]}


@pytest.fixture(scope='module', autouse=True)
def _no_miopen():
    prev = torch.backends.cudnn.enabled
    torch.backends.cudnn.enabled = False
    yield
    torch.backends.cudnn.enabled = prev


def fallback_key(o):
    """The kernel a forced variant runs on conv op o where its form does not apply: the register-staged tile kernel by
    output width (csrc/conv_f16.hip pick_tile, the rows of conv_f16_launch.h tile_rows).  (The kernels of forced variant
    1 itself are another family: without a residual, csrc/conv.hip launch_conv sends it to that file's generic kernel.)"""
    bn, wm = (32, 4) if o['cout'] <= 32 else (64, 2) if o['cout'] <= 64 else (128, 2)
    one = o.get('k', 1) == 1 and o.get('s', 1) == 1 and o.get('pad', 0) == 0
    return f'conv_f16_kernel<128, {bn}, {wm}, {"true" if one else "false"}, false, 1, false>'


def launched_elsewhere(plan, B, H, W):
    """The conv ops (MP-folded ones aside: their kernel is the pooled tile whatever the variant) on which the variants
    now set launch a kernel other than the fallback (a dry run)."""
    ks = plan.op_kernels(B, H, W)
    return [i for i, o in enumerate(plan.graph.ops) if o['kind'] == L.OP_CONV and not o.get('pool') and
            any(kernel_key(k) != fallback_key(o) for k in ks[i])]


@pytest.mark.parametrize('name,B,H,W', NETWORKS)
def test_every_conv_variant(name, B, H, W):
    m = fresh_model(name).to(DEV).half()
    plan = m.plan()
    x = frames(B, H, W, seed=31).to(DEV).half()
    convs = [i for i, o in enumerate(plan.graph.ops) if o['kind'] == L.OP_CONV]
    dets = [i for i, o in enumerate(plan.graph.ops) if o['kind'] == L.OP_DETECT]
    lines = []
    LAUNCHED[name] = {}
    for v in CONV_VARIANTS + DET_VARIANTS:
        for i in (dets if v in DET_VARIANTS else convs):
            plan.set_op_variant(i, v)
        if v in CONV_VARIANTS:
            LAUNCHED[name][v] = launched_elsewhere(plan, B, H, W)
            lines.append(f'variant {v}: a kernel other than the fallback on ops {LAUNCHED[name][v]}')
        z, xs = plan.forward(x)
        torch.cuda.synchronize()
        out = check_ops(plan, x, B, H, W, raw=xs, z=z)
        lines.append(f'variant {v}: ' + kernel_summary(out))
        if v in DET_VARIANTS:
            lines.append(_check_no_raw_call(plan, x, B, H, W, v, dets, z))
        for i in (dets if v in DET_VARIANTS else convs):
            plan.set_op_variant(i, 0)
    print('\n' + '\n'.join(lines))


def test_variants_that_launch_nowhere():
    """Over both networks of test_every_conv_variant (a network that test has not run in this session is dry-run here),
    the variants whose own kernel launches on no conv op are exactly LAUNCH_NOWHERE."""
    for name, B, H, W in NETWORKS:
        if name in LAUNCHED:
            continue
        plan = fresh_model(name).to(DEV).half().plan()
        convs = [i for i, o in enumerate(plan.graph.ops) if o['kind'] == L.OP_CONV]
        LAUNCHED[name] = {}
        for v in CONV_VARIANTS:
            for i in convs:
                plan.set_op_variant(i, v)
            LAUNCHED[name][v] = launched_elsewhere(plan, B, H, W)
    nowhere = [v for v in CONV_VARIANTS if not any(LAUNCHED[name][v] for name, *_ in NETWORKS)]
    assert nowhere == LAUNCH_NOWHERE, nowhere


def _check_no_raw_call(plan, x, B, H, W, v, dets, z_raw):
    """A forced Detect variant through the call without raw logits (the benchmark's): the forward above returns
    them, and with a raw pointer 94 is not admitted (det_pring_supported) and runs the 64 x 256 ring.  Here 94 must
    launch conv_det_pring_kernel on every level (both shapes of this test meet det_pring_supported: every level's
    size, first z row and the rows per image are multiples of 4), and every variant's z must pass the float64
    reference that needs no raw logits (opcheck.check_detect_z) and equal the raw path's z bit for bit."""
    ks = plan.op_kernels(B, H, W)
    for i in dets:
        head = [kernel_key(k) for k in ks[i]]
        assert len(head) == 1, (v, i, head)
        if v == 94:
            assert head[0] == 'conv_det_pring_kernel<0>', (v, i, head)
        else:
            assert not head[0].startswith('conv_det_'), (v, i, head)
    N = plan.num_rows(H, W)
    zbuf = torch.full((B + 2, N, plan.no), float('nan'), dtype=torch.float32, device=DEV)
    z = zbuf[1:-1]
    plan.forward_into(x, z)
    torch.cuda.synchronize()
    assert torch.isnan(zbuf[0]).all() and torch.isnan(zbuf[-1]).all(), f'variant {v}: z written outside its images'
    ratios = check_detect_z(plan, B, H, W, z)
    assert torch.equal(z, z_raw), f'variant {v}: z without raw logits differs from the raw path\'s z'
    heads = ', '.join(f'level {lvl}: {kernel_key(ks[i][0])} {r:.3g}' for lvl, (i, r) in sorted(ratios.items()))
    return f'variant {v} without raw logits (worst z ratio to the bound): {heads}'


# A net with the shapes the fragment kernels mask: 3x3 layers with cout % 32 == 16 (cout = 80:
# the permlane16 pair store of the 32-channel pair 64..95 is half masked), stride-2 layers with cin 64
# and 128 (conv_s2.hip's two weight layouts), and batches with a partial trailing 4-image group after
# full ones (B = 5, 6).  ADVICE r5: 1x1 layers with the register-weight kernel's input widths (cin 128 /
# 256 / 512, conv_w1.hip) and outputs of 80 / 144 channels (cout % 32 == 16: masked pair store), so the
# forced w1 variants really launch on a half-masked N slice and a partial pixel tile (layers 8, 10, 12).
RAGGED = {'nc': 3, 'depth_multiple': 1.0, 'width_multiple': 1.0,
          'anchors': [[10, 13, 16, 30, 33, 23], [30, 61, 62, 45, 59, 119], [116, 90, 156, 198, 373, 326]],
          'backbone': [[-1, 1, 'Conv', [32, 3, 1]],    # 0  @1
                       [-1, 1, 'Conv', [64, 3, 2]],    # 1  @2
                       [-1, 1, 'Conv', [80, 3, 1]],    # 2  lr, cin 64 -> 80
                       [-1, 1, 'Conv', [64, 1, 1]],    # 3
                       [-1, 1, 'Conv', [80, 3, 2]],    # 4  @4: s2, cin 64 -> 80
                       [-1, 1, 'Conv', [128, 1, 1]],   # 5
                       [-1, 1, 'Conv', [80, 3, 2]],    # 6  @8: s2, cin 128 -> 80
                       [-1, 1, 'Conv', [128, 1, 1]],   # 7
                       [-1, 1, 'Conv', [80, 1, 1]],    # 8  w1, cin 128 -> 80
                       [-1, 1, 'Conv', [256, 1, 1]],   # 9
                       [-1, 1, 'Conv', [144, 1, 1]],   # 10 w1, cin 256 -> 144
                       [-1, 1, 'Conv', [512, 1, 1]],   # 11
                       [-1, 1, 'Conv', [80, 1, 1]],    # 12 w1, cin 512 -> 80
                       [-1, 1, 'Conv', [128, 1, 1]],   # 13
                       [-1, 1, 'Conv', [80, 3, 1]],    # 14 lr, cin 128 -> 80 (P3)
                       [-1, 1, 'Conv', [64, 1, 1]],    # 15
                       [-1, 1, 'Conv', [80, 3, 2]],    # 16 @16: s2, cin 64 (P4)
                       [-1, 1, 'Conv', [128, 1, 1]],   # 17
                       [-1, 1, 'Conv', [96, 3, 2]]],   # 18 @32: s2, cin 128 (P5)
          'head': [[[14, 16, 18], 1, 'Detect', ['nc', 'anchors']]]}
# register-weight 1x1 configurations (conv_w1.hip w1_rows) -> the input width each one takes
W1_CIN = {290: 128, 291: 256, 292: 512, 293: 256, 294: 128, 295: 512, 302: 256, 303: 256}


@pytest.mark.parametrize('B', [5, 6])
def test_fragment_kernels_ragged(B):
    """The fragment kernels (conv_lr.hip 270-279, conv_s2.hip 280-288, conv_w1.hip 290-295, 302-303) on partial
    trailing image groups / pixel tiles and half-masked channel pairs, op by op against fp32 torch.  A forced
    w1 variant must actually launch conv1x1_rw_kernel on every 1x1 layer of its input width (no silent
    fallback to the tuned kernel)."""
    import copy
    from models.yolo import Model
    from yv7.synthetic import synthetic_state_dict
    m = Model(copy.deepcopy(RAGGED))
    m.load_state_dict(synthetic_state_dict(m, seed=3, calib_hw=256))
    m = m.float().eval().fuse().to(DEV).half()
    plan = m.plan()
    H = W = 256
    x = frames(B, H, W, seed=7).to(DEV).half()
    convs = [i for i, o in enumerate(plan.graph.ops) if o['kind'] == L.OP_CONV]
    lines = []
    for v in [0, 270, 271, 272, 273, 274, 275, 276, 277, 278, 279, 280, 281, 282, 283, 284, 285, 286, 287, 288,
              290, 291, 292, 293, 294, 295, 302, 303]:
        for i in convs:
            plan.set_op_variant(i, v)
        if v in W1_CIN:
            ks = plan.op_kernels(B, H, W)
            want = [i for i in convs if plan.graph.ops[i].get('k', 1) == 1 and plan.graph.ops[i]['cin'] == W1_CIN[v]
                    and plan.graph.ops[i]['cout'] % 32 == 16]
            assert want, f'variant {v}: no 1x1 layer with cin {W1_CIN[v]} and a half-masked channel pair'
            for i in want:
                assert any('conv1x1_rw_kernel' in k for k in ks[i]), (v, i, ks[i])
        z, xs = plan.forward(x)
        torch.cuda.synchronize()
        out = check_ops(plan, x, B, H, W, raw=xs, z=z)
        lines.append(f'variant {v}: ' + kernel_summary(out))
        for i in convs:
            plan.set_op_variant(i, 0)
    print('\n' + '\n'.join(lines))


def test_variant_api_rejects_hooks():
    """Microbenchmark hooks (which skip work on purpose) and unchecked experiment schedules (the
    round-2 ws64 / 8-phase scheduling experiments 18-19, 241-255) cannot be forced through the ABI (17 is
    now the 8-wave ws64 form, a kernel configuration)."""
    m = fresh_model('yolov7-tiny').to(DEV).half()
    plan = m.plan()
    conv = next(i for i, o in enumerate(plan.graph.ops) if o['kind'] == L.OP_CONV)
    for v in (12, 13, 14, 16, 18, 19, 90, 91, 93, 94, 298, 160, 190, 105, 211, 221, 233, 237, 238, 240, 241,
              248, 255, 259, 260, 261, 263, 289, 296, 299, 300, 301, 304, 911):
        with pytest.raises(RuntimeError):
            plan.set_op_variant(conv, v)
    # the Detect op: the detbench hooks (91, 93, 95, 96, 98 reach launch_det_pring) are refused, the
    # alternative heads the suite checks (92, 94, 97, 99) are accepted
    det = next(i for i, o in enumerate(plan.graph.ops) if o['kind'] == L.OP_DETECT)
    for v in (91, 93, 95, 96, 98):
        with pytest.raises(RuntimeError):
            plan.set_op_variant(det, v)
    for v in DET_VARIANTS:
        plan.set_op_variant(det, v)
    plan.set_op_variant(det, 0)
    with pytest.raises(RuntimeError):
        plan.set_op_variant(len(plan.graph.ops) + 3, 0)
