"""Parity at the bench's own configuration: yolov7 (P5) 640x640, batch 32 — BASELINE configs[1].

Kernel choice in libyv7 depends on the tile count of each layer (csrc/conv_f16.hip pick_tuned /
choose), so the kernels behind the headline number (the persistent weight-stationary 3x3, the 256 x
256 persistent rings on 3x3 and 1x1 layers, split-K on the 20 x 20 layers, the pooled 1x1, the fused
stem, the Detect epilogue with row scores) run only at this batch and resolution.  Here the exact
bench dispatch runs and is checked three ways:
  * every op against a plain PyTorch fp32 reference of the same op on the op's own input
    (tests/opcheck.py: one fp16 ulp), all 32 images;
  * the whole network against the CPU oracle (the reference's forward_once restated) on images
    0, 15 and 31 (images are independent), layer by layer: fp16 within the reference's own half()
    error (oracle half-storage emulation) or 5e-3 rms, fp32 by the check_z criterion;
  * the serving schedule (3 batches in flight, bench.py's default) bit-identical to serial batches,
    and its NMS bit-exact against the oracle's NMS on the same z.
Reference computations: models/common.py:110-111 (Conv.fuseforward), 498-500 (RepConv),
models/yolo.py:42-63 (Detect), utils/general.py:628-720 (NMS).
"""
import pytest
import torch

from helpers import fresh_model, frames, oracle_net
from opcheck import check_ops, kernel_summary, rms_rel
from parity import check_z

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
B, H, W = 32, 640, 640
PICK = [0, 15, 31]


@pytest.fixture(scope='module', autouse=True)
def _no_miopen():
    prev = torch.backends.cudnn.enabled
    torch.backends.cudnn.enabled = False   # torch references use native kernels (no run-time compiles)
    yield
    torch.backends.cudnn.enabled = prev


RB_SENT = 0x7FA5A5A5   # a NaN bit pattern no row record holds


def sentinel_buffers(Bq, N, no):
    """z filled with NaN and row records filled with RB_SENT: torch.empty could hand back the block of an earlier,
    identical z from the caching allocator, and rows a head never wrote would go unnoticed."""
    z = torch.full((Bq, N, no), float('nan'), dtype=torch.float32, device=DEV)
    rb = torch.full((Bq, N, 4), RB_SENT, dtype=torch.int32, device=DEV).view(torch.float32)
    return z, rb


def assert_all_written(z, rb):
    assert torch.isfinite(z).all(), f'{int((~torch.isfinite(z)).sum())} z elements not written / not finite'
    left = int((rb.view(torch.int32) == RB_SENT).sum())
    assert left == 0, f'{left} row-record words left at the sentinel'


@pytest.fixture(scope='module')
def batch():
    return frames(B, H, W, seed=21)


def test_bench_config_fp16_every_op(batch):
    m = fresh_model('yolov7').to(DEV).half()
    plan = m.plan()
    x = batch.to(DEV).half()
    N = plan.num_rows(H, W)
    # the bench's call: z + row-score records, no raw logits
    z1, rb = sentinel_buffers(B, N, plan.no)
    plan.forward_into(x, z1, rowbest=rb)
    z, xs = plan.forward(x)
    torch.cuda.synchronize()
    assert_all_written(z1, rb)
    assert torch.equal(z, z1), 'raw-logit output changed z'
    out = check_ops(plan, x, B, H, W, raw=xs, z=z)
    print('\nyolov7 640 bs32 fp16: ' + kernel_summary(out))
    # the forward's own row records equal what NMS derives from z
    obj = z[..., 4]
    best, cls = (z[..., 5:] * obj[..., None]).max(-1)
    assert torch.equal(rb[..., 0], obj) and torch.equal(rb[..., 1], best)
    assert torch.equal(rb[..., 2].view(torch.int32), cls.to(torch.int32))

    # layer by layer against the oracle on three of the 32 images
    from oracle import yolo_ref
    net, fused = oracle_net('yolov7')
    xp = batch[PICK]
    (zr, _), outs = yolo_ref.forward(net, fused, xp, return_all=True)
    (ze, _), outs16 = yolo_ref.forward(net, fused, xp, return_all=True, half_storage=True)
    worst = (0.0, None)
    for i in sorted(plan.graph.layer_tensor):
        ref = outs[i]
        if not isinstance(ref, torch.Tensor):
            continue
        got = plan.layer_output(i, B, H, W)[PICK].cpu()
        e = rms_rel(got, ref)
        bar = max(5e-3, 1.5 * rms_rel(outs16[i], ref))
        assert e <= bar, f'layer {i}: rms-rel {e:.3g} > {bar:.3g}'
        worst = max(worst, (e, i))
    print(f'oracle images {PICK}: worst layer rms-rel {worst[0]:.3g} at layer {worst[1]}')
    zc = z[PICK].cpu()
    sc = zr.abs().clamp(min=1)
    print(f'z vs fp32 oracle: coord rel {((zc - zr).abs() / sc)[..., :4].max():.3g} '
          f'(reference half() emulation {((ze - zr).abs() / sc)[..., :4].max():.3g})')


def test_bench_config_fp32(batch):
    m = fresh_model('yolov7').to(DEV)
    plan = m.plan()
    x = batch.to(DEV)
    z, xs = plan.forward(x)
    torch.cuda.synchronize()
    out = check_ops(plan, x, B, H, W, raw=xs, z=z)
    print('\nyolov7 640 bs32 fp32: ' + kernel_summary(out))
    from oracle import yolo_ref
    net, fused = oracle_net('yolov7')
    xp = batch[PICK]
    zr, _ = yolo_ref.forward(net, fused, xp)
    z64, _ = yolo_ref.forward64(net, fused, xp)
    print(check_z(z[PICK], zr, z64, f'yolov7 640 bs32 fp32, images {PICK}'))


def test_bench_config_inflight_nms(batch):
    """bench.py's schedule: 3 batches of 32 in flight (yv7.runtime.Inflight) == serial, bit for bit;
    the NMS of each batch == the oracle's NMS on the same z."""
    from oracle import nms_ref
    from utils.general import nms_batched
    from yv7.runtime import Inflight
    m = fresh_model('yolov7').to(DEV).half()
    plan = m.plan()
    xs = [batch.to(DEV).half(), batch.flip(3).to(DEV).half(), frames(B, H, W, seed=22).to(DEV).half(),
          frames(B, H, W, seed=23).to(DEV).half()]
    want = []
    for i, x in enumerate(xs):
        z, _ = plan.forward(x, want_raw=False)
        det, src, cnt = nms_batched(z, 0.25, 0.45)
        want.append((det.clone(), src.clone(), cnt.clone()))
        if i == 0:
            out_r, rows_r = nms_ref.non_max_suppression(z.cpu(), 0.25, 0.45, return_rows=True)
            c = cnt.cpu().tolist()
            for b in range(B):
                assert torch.equal(src[b, :c[b]].cpu(), rows_r[b]) and torch.equal(det[b, :c[b]].cpu(), out_r[b]), b
    run = Inflight(plan, B, H, W, streams=3)
    hs = [run.submit(x) for x in xs[:3]]
    got = [tuple(t.clone() for t in run.result(hs[0]))]
    hs.append(run.submit(xs[3]))
    got += [tuple(t.clone() for t in run.result(h)) for h in hs[1:]]
    run.close()
    for i, ((d, s, c), (dw, sw, cw)) in enumerate(zip(got, want)):
        assert torch.equal(c, cw), i
        for b in range(B):
            n = int(cw[b])
            assert torch.equal(s[b, :n], sw[b, :n]) and torch.equal(d[b, :n], dw[b, :n]), (i, b)


def test_w6_config_fp16_every_op():
    """BASELINE configs[3]: yolov7-w6 (P6) 1280x1280 at batch 8 — the bench line's exact dispatch
    (kernel choice depends on each layer's tile count: split-K in four on 512->512 @20, the persistent
    rings on the 1280 / 640 / 320 stages, ReOrg fused into the input packing, the 4-level Detect
    head).  Every op against a plain PyTorch fp32 reference on its own input (tests/opcheck.py), then
    the whole network against the CPU oracle on images 0 and 7, layer by layer.
    Reference: cfg/deploy/yolov7-w6.yaml; ReOrg models/common.py:48-53; Detect models/yolo.py:42-63."""
    Bw, Hw = 8, 1280
    xb = frames(Bw, Hw, Hw, seed=25)
    m = fresh_model('yolov7-w6').to(DEV).half()
    plan = m.plan()
    x = xb.to(DEV).half()
    N = plan.num_rows(Hw, Hw)
    z1, rb = sentinel_buffers(Bw, N, plan.no)
    plan.forward_into(x, z1, rowbest=rb)       # bench.py's call
    z, xs = plan.forward(x)
    torch.cuda.synchronize()
    assert_all_written(z1, rb)
    assert torch.equal(z, z1), 'raw-logit output changed z'
    out = check_ops(plan, x, Bw, Hw, Hw, raw=xs, z=z)
    print('\nyolov7-w6 1280 bs8 fp16: ' + kernel_summary(out))
    from oracle import yolo_ref
    net, fused = oracle_net('yolov7-w6')
    pick = [0, 7]
    xp = xb[pick]
    (zr, _), outs = yolo_ref.forward(net, fused, xp, return_all=True)
    (ze, _), outs16 = yolo_ref.forward(net, fused, xp, return_all=True, half_storage=True)
    worst = (0.0, None)
    for i in sorted(plan.graph.layer_tensor):
        ref = outs[i]
        if not isinstance(ref, torch.Tensor):
            continue
        got = plan.layer_output(i, Bw, Hw, Hw)[pick].cpu()
        e = rms_rel(got, ref)
        bar = max(5e-3, 1.5 * rms_rel(outs16[i], ref))
        assert e <= bar, f'layer {i}: rms-rel {e:.3g} > {bar:.3g}'
        worst = max(worst, (e, i))
    print(f'oracle images {pick}: worst layer rms-rel {worst[0]:.3g} at layer {worst[1]}')
    zc = z[pick].cpu()
    sc = zr.abs().clamp(min=1)
    print(f'z vs fp32 oracle: coord rel {((zc - zr).abs() / sc)[..., :4].max():.3g} '
          f'(reference half() emulation {((ze - zr).abs() / sc)[..., :4].max():.3g})')


def test_tiny_config_fp16_every_op(batch):
    """yolov7-tiny 640 at batch 32 (`bench.py --model yolov7-tiny`, the tiny line in profiles/): its exact
    dispatch — which differs from the small-frame one the forced-variant tests see (round 5: the 8-wave
    weight-stationary 3x3 takes its 64->64 @80 layers from 800 tiles) — every op against a plain PyTorch
    fp32 reference on its own input (tests/opcheck.py), plus the row records vs z.
    Reference: cfg/deploy/yolov7-tiny.yaml; models/common.py:110-111; models/yolo.py:42-63."""
    m = fresh_model('yolov7-tiny').to(DEV).half()
    plan = m.plan()
    x = batch.to(DEV).half()
    N = plan.num_rows(H, W)
    z1, rb = sentinel_buffers(B, N, plan.no)
    plan.forward_into(x, z1, rowbest=rb)
    z, xs = plan.forward(x)
    torch.cuda.synchronize()
    assert_all_written(z1, rb)
    assert torch.equal(z, z1), 'raw-logit output changed z'
    out = check_ops(plan, x, B, H, W, raw=xs, z=z)
    print('\nyolov7-tiny 640 bs32 fp16: ' + kernel_summary(out))
    obj = z[..., 4]
    best, cls = (z[..., 5:] * obj[..., None]).max(-1)
    assert torch.equal(rb[..., 0], obj) and torch.equal(rb[..., 1], best)
    assert torch.equal(rb[..., 2].view(torch.int32), cls.to(torch.int32))


def test_fp8_config_every_op(batch):
    """BASELINE configs[4]: the product fp8 plan at yolov7 640 batch 32 (bench.py --dtype fp8).  The fp16
    ops against plain PyTorch fp32 references (tests/opcheck.py), every fp8 op against the restatement of
    its arithmetic applied to the very fp16 input it read (e4m3 input on the op's power-of-two scale, the
    plan's per-channel e4m3 weights, fp32 accumulation, bias, activation; oracle.yolo_ref.fp8_e4m3 =
    torch.float8_e4m3fn rounding), output within 2e-3 of max|y|."""
    import torch.nn.functional as F

    import plan_interp
    from oracle import yolo_ref
    from yv7 import _lib as L
    from yv7.runtime import Plan
    m = fresh_model('yolov7').to(DEV).half()
    plan = Plan.fp8_from_model(m, DEV)
    x = batch.to(DEV).half()
    N = plan.num_rows(H, W)
    z, rb = sentinel_buffers(B, N, plan.no)
    plan.forward_into(x, z, rowbest=rb)
    z2, xs = plan.forward(x)
    torch.cuda.synchronize()
    assert_all_written(z, rb)
    assert torch.equal(z, z2)
    out = check_ops(plan, x, B, H, W, raw=xs, z=z2, skip_fp8=True)
    blob = plan.graph.weight_blob()
    acts = {L.ACT_SILU: F.silu, L.ACT_LEAKY: lambda t: F.leaky_relu(t, 0.1), L.ACT_NONE: lambda t: t}
    worst, n = 0.0, 0
    for o in plan.graph.ops:
        if o.get('wfmt', 0) != L.WFMT_FP8:
            continue
        xin = plan.tensor_view(o['src'], B, H, W)[..., o['src_coff']:o['src_coff'] + o['cin']].float()
        xq = yolo_ref.fp8_e4m3(xin / o['xscale']) * o['xscale']
        w = plan_interp._weights_f8(blob, o['w_off'], o['cout'], o['cin'], o['s_off']).reshape(o['cout'], -1).to(DEV)
        b = plan_interp._bias(blob, o['b_off'], o['cout']).to(DEV)
        want = acts[o['act']](xq.reshape(-1, o['cin']) @ w.t() + b)
        got = plan.tensor_view(o['dst'], B, H, W)[..., o['dst_coff']:o['dst_coff'] + o['cout']].float()
        err = ((got.reshape(-1, o['cout']) - want).abs().max() / want.abs().max().clamp(min=1e-3)).item()
        assert err < 2e-3, f'fp8 op {o["cin"]}->{o["cout"]}: max-norm rel err {err:.3g}'
        worst = max(worst, err)
        n += 1
    print(f'\nyolov7 640 bs32 fp8: {kernel_summary(out)} (fp16 ops); {n} fp8 ops, worst max-norm rel err {worst:.3g}')
    assert n >= 10


# The end-of-round bench lines measured mAP@0.5 0.9764 (round 3, BENCH_r03.json) and 0.984 (round 4,
# BENCH_r04.json) on these 16 frames; every later change of summation order (sibling merges, the dual 1x1,
# the low-resolution 3x3 kernel, the register-weight stride-2 kernel) must show its parity cost against
# the latest value (ratcheted to round 4 by VERDICT r4 item 5).
MAP50_REF = 0.984


@pytest.mark.gpu
def test_bench_dispatch_map_parity_guard():
    """The bench line's parity half on the bench's exact dispatch (yolov7 640, the 16 parity frames in a
    batch of 32, fp16): mAP@0.5 of the GPU detections against the oracle's fp32 detections must stay
    within 0.005 of round 4's 0.984 (bench.py map_parity; general.py:628-720, test.py:126)."""
    import bench
    from yv7.runtime import Plan
    net, fused = oracle_net('yolov7')
    plan = Plan.from_model(fresh_model('yolov7'), DEV, torch.float16)
    r = bench.map_parity(net, fused, 640, plan, DEV, frames=16, batch=32)
    print(f"\nbench-dispatch mAP@0.5 {r['map50']:.4f} (round 4: {MAP50_REF}), mAP@.5:.95 {r['map50_95']:.4f}")
    assert r['batch'] == 32
    assert r['map50'] >= MAP50_REF - 0.005
