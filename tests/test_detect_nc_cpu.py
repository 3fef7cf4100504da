"""Custom class counts without a device: the compiled plans of nc = 83 / nc = 1 models carry a DETECT op of
na * (nc + 5) channels and, executed op by op on the CPU (tests/plan_interp.py), reproduce the oracle's z; and
yv7_plan_create's validation (which runs before any device is touched, tests/test_plan_validate.py) names the
head limits — na <= 4 (ConvParams::anchor holds 8 floats) and nc <= 128 (the NMS's bound; the widest tile of
conv_det_nc_kernel, 144 channels per anchor, covers it) — for an fp16 plan past them."""
import pytest
import torch

from test_plan_validate import create, network
from yv7 import _lib as L
from yv7.graph import compile_model


@pytest.mark.parametrize('nc', [83, 1])
@pytest.mark.parametrize('dtype', [L.DT_F32, L.DT_F16])
def test_compiled_plan_of_a_custom_nc_model(nc, dtype):
    import plan_interp
    from helpers import frames
    from models.yolo import Model
    from oracle import yolo_ref
    from yv7.synthetic import synthetic_state_dict
    m = Model('yolov7-tiny', nc=nc)
    assert m.yaml['nc'] == nc and len(m.names) == nc
    sd = synthetic_state_dict(m, seed=0)
    net = yolo_ref.parse(m.yaml)
    fused = yolo_ref.fuse(net, sd)
    m.load_state_dict(sd)
    g = compile_model(m.float().eval().fuse(), dtype)
    dets = [o for o in g.ops if o['kind'] == L.OP_DETECT]
    assert (g.na, g.no) == (3, nc + 5) and len(dets) == 3 and all(o['cout'] == 3 * (nc + 5) for o in dets)
    x = frames(1, 64, 64)
    with torch.no_grad():
        want = yolo_ref.forward(net, fused, x)[0]
        got = plan_interp.run(g, x)
    assert got.shape == want.shape == (1, 3 * (64 + 16 + 4), nc + 5)
    if dtype == L.DT_F32:   # tests/test_graph.py's bar for the fp32 plan
        torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-3)
    else:                   # fp16 storage: the fp16 plans' rms bar (tests/test_gpu_forward.py)
        from opcheck import rms_rel
        assert rms_rel(got, want) < 0.05


def _na(net, tensors, ops): net['na'], ops[2].cout = 5, 30
def _no(net, tensors, ops): net['no'], ops[2].cout = 5 + 129, 5 + 129   # noqa: E302


@pytest.mark.parametrize('mutate', [_na, _no], ids=['na', 'no'])
def test_fp16_plan_past_the_head_limits(mutate):
    net, tensors, ops = network()
    assert net['dtype'] == L.DT_F16
    mutate(net, tensors, ops)
    rc, msg = create(net, tensors, ops)
    assert rc == -1 and 'na<=4' in msg and 'nc<=128' in msg, (rc, msg)


def test_fp16_plan_at_the_head_limits_is_not_an_argument_error():
    """na = 4 and nc = 128 pass the validation: 0 with a GPU, the first device call's error without one."""
    net, tensors, ops = network()
    net['na'], ops[2].cout = 4, 24
    rc, msg = create(net, tensors, ops)
    assert rc != -1 or not msg.startswith('yv7_plan_create:'), (rc, msg)
