"""Model(cfg, ch=C) without a GPU: the parse against the oracle's, what the graph compiler lowers the front end to
for each channel count, conv A's packed row for the fused stem, the entry points that refuse such a model, and
yv7_plan_create's checks of the INPUT op (all before any device is touched).

Front ends (yv7/graph.py _STEMS): fp16 plans of a model without a leading ReOrg run layers 0-1 as one STEM op for
C in {1, 2, 3, 4} (the stem's LDS patch has four channel slots per pixel); C > 4, a ReOrg model with C != 3 and every
fp32 plan lower to INPUT + CONV ops, the INPUT op's cout the channels it packs (C, or 4 C behind the ReOrg)."""
import functools

import pytest
import torch

import test_plan_validate as V
from models.yolo import Model
from oracle import yolo_ref
from yv7 import _lib as L
from yv7.arch import get_cfg
from yv7.graph import compile_model

REFUSAL = 'this entry point loads 3-channel images; call the model on a \\[B,C,H,W\\] tensor'


@functools.lru_cache(maxsize=None)
def model(name, C):
    torch.manual_seed(0)
    return Model(name, ch=C).float().fuse().eval()


@pytest.mark.parametrize('C', [1, 4])
@pytest.mark.parametrize('name', ['yolov7-tiny', 'yolov7', 'yolov7-w6'])
def test_parse_matches_the_oracle(name, C):
    m = model(name, C)
    net = yolo_ref.parse(get_cfg(name), ch_in=C)
    assert len(m.model) == len(net.layers) and m.save == net.save
    assert [float(s) for s in m.stride] == net.stride
    assert m.yaml['ch'] == C
    if name == 'yolov7-w6':   # ReOrg, then the first conv on the 4 C reorganised channels
        assert net.layers[0].c1 == C and net.layers[1].c1 == 4 * C and m.model[1].conv.in_channels == 4 * C
    else:
        assert net.layers[0].c1 == C and m.model[0].conv.in_channels == C
        assert m.model[1].conv.in_channels == net.layers[1].c1 == m.model[0].conv.out_channels


@pytest.mark.parametrize('C', [1, 2, 4])
@pytest.mark.parametrize('name,sa', [('yolov7-tiny', 2), ('yolov7', 1)])
def test_fp16_plan_fuses_the_stem(name, sa, C):
    m = model(name, C)
    g = compile_model(m, L.DT_F16)
    st = g.ops[0]
    assert g.in_channels == C
    assert st['kind'] == L.OP_STEM and (st['cin'], st['cout'], st['cout2'], st['s']) == (C, 32, 64, sa)
    assert not any(o['kind'] == L.OP_INPUT for o in g.ops)
    # conv A's packed row: the plain [cout][kh][kw][C] reshape of the fused weight (k = tap * C + ci), one 64-wide row
    w, _ = m.model[0].fused_weight_bias()
    want = torch.zeros(32, 64, dtype=torch.float16)
    want[:, :9 * C] = w.permute(0, 2, 3, 1).reshape(32, 9 * C).half()
    blob = g.weight_blob()
    got = blob[st['w_off']:st['w_off'] + 32 * 64 * 2].view(torch.float16).view(32, 64)
    assert torch.equal(got, want)
    # conv B is packed as before: [64][9 * 32 -> 320]
    wb, _ = m.model[1].fused_weight_bias()
    gotb = blob[st['w2_off']:st['w2_off'] + 64 * 320 * 2].view(torch.float16).view(64, 320)
    assert torch.equal(gotb[:, :288], wb.permute(0, 2, 3, 1).reshape(64, 288).half()) and not gotb[:, 288:].any()


def test_three_channels_lower_as_before():
    """C = 3 is the same STEM op as ever (tests/golden/graph_plans.txt pins the whole plans)."""
    g = compile_model(model('yolov7-tiny', 3), L.DT_F16)
    assert g.in_channels == 3 and (g.ops[0]['kind'], g.ops[0]['cin']) == (L.OP_STEM, 3)


def test_five_channels_lower_to_input_and_conv():
    g = compile_model(model('yolov7-tiny', 5), L.DT_F16)
    assert g.in_channels == 5
    assert (g.ops[0]['kind'], g.ops[0]['k'], g.ops[0]['cout']) == (L.OP_INPUT, 1, 5)
    assert (g.ops[1]['kind'], g.ops[1]['cin'], g.ops[1]['src']) == (L.OP_CONV, 8, g.ops[0]['dst'])
    assert g.tensors[g.ops[0]['dst']] == [8, 0]
    assert not any(o['kind'] == L.OP_STEM for o in g.ops)


@pytest.mark.parametrize('dtype', [L.DT_F16, L.DT_F32], ids=['fp16', 'fp32'])
def test_reorg_model_with_one_channel_is_not_fused(dtype):
    g = compile_model(model('yolov7-w6', 1), dtype)
    o = g.ops[0]
    assert (o['kind'], o['k'], o['cout']) == (L.OP_INPUT, 2, 4) and g.tensors[o['dst']][1] == 1
    assert not any(q['kind'] == L.OP_STEM for q in g.ops)
    assert g.ops[1]['kind'] == L.OP_CONV and g.ops[1]['cin'] == (8 if dtype == L.DT_F16 else 4)


@pytest.mark.parametrize('name,C', [('yolov7-tiny', 1), ('yolov7-tiny', 4), ('yolov7', 1), ('yolov7', 4)])
def test_fp32_plans_pack_the_input(name, C):
    g = compile_model(model(name, C), L.DT_F32)
    assert (g.ops[0]['kind'], g.ops[0]['k'], g.ops[0]['cout']) == (L.OP_INPUT, 1, C)
    assert g.ops[1]['kind'] == L.OP_CONV and g.ops[1]['cin'] == 4
    assert not any(o['kind'] == L.OP_STEM for o in g.ops)


def test_cfg_dict_with_ch_gives_the_same_graph():
    cfg = get_cfg('yolov7-tiny')
    assert 'ch' not in cfg
    cfg['ch'] = 1
    torch.manual_seed(0)
    m = Model(cfg).float().fuse().eval()   # no ch= argument: the cfg's own ch
    assert m.yaml['ch'] == 1 and m.model[0].conv.in_channels == 1
    for dtype in (L.DT_F16, L.DT_F32):
        a, b = compile_model(m, dtype), compile_model(model('yolov7-tiny', 1), dtype)
        assert a.ops == b.ops and a.tensors == b.tensors and a.in_channels == b.in_channels == 1
    # the cfg's own ch wins over the argument, as in the reference's constructor (models/yolo.py:521)
    assert Model(dict(cfg), ch=3).model[0].conv.in_channels == 1


def test_op_costs_count_the_image_planes():
    """Plan.op_costs' image bytes are B * C * H * W (on a stand-in plan: no device)."""
    from yv7.runtime import Plan
    for C, dtype in ((1, L.DT_F16), (4, L.DT_F16), (5, L.DT_F16), (1, L.DT_F32)):
        g = compile_model(model('yolov7-tiny', C), dtype)
        p = Plan.__new__(Plan)
        p.graph, p.dtype = g, dtype
        B, H, W, es = 2, 64, 96, 2 if dtype == L.DT_F16 else 4
        kind, flops, by = Plan.op_costs(p, B, H, W, x_bytes=2)[0]
        if kind == L.OP_STEM:
            assert by == B * C * H * W * 2 + 2 * B * (H // 2) * (W // 2) * 32 * es + B * (H // 4) * (W // 4) * 64 * es
            assert flops == 2.0 * B * (H // 2) * (W // 2) * 32 * 9 * C + 2.0 * B * (H // 4) * (W // 4) * 64 * 9 * 32
        else:
            assert kind == L.OP_INPUT and by == B * C * H * W * 2 + B * H * W * g.tensors[0][0] * es


def test_autoshape_refuses_on_the_cpu():
    """Model.autoshape() and autoShape(model) on a CPU model: refused before any device use."""
    from models.common import autoShape
    m = model('yolov7-tiny', 1)
    with pytest.raises(RuntimeError, match=REFUSAL):
        m.autoshape()
    with pytest.raises(RuntimeError, match=REFUSAL):
        autoShape(m)
    assert isinstance(model('yolov7-tiny', 3).autoshape(), autoShape)


def test_ensemble_of_such_models_is_refused_too():
    from models.experimental import Ensemble
    from utils.general import check_three_channels
    e = Ensemble([model('yolov7-tiny', 3), model('yolov7-tiny', 1)])
    with pytest.raises(RuntimeError, match=REFUSAL):
        check_three_channels(e)
    check_three_channels(Ensemble([model('yolov7-tiny', 3)]))


def _with_input(**kw):
    def mutate(net, tensors, ops):
        for k, v in kw.items():
            setattr(ops[0], k, v)
    return mutate


def test_plan_create_input_refusals_are_host_only():
    """The INPUT op's channel count (cout) is checked with the rest of the descriptor, before any device is touched:
    each refusal is YV7_E_ARG with its own text; tests/test_plan_validate.py's descriptor, whose tensor 0 has 8
    channels.  cout = 0, from a descriptor written before the field was read, still stands for the 3-channel image."""
    seen = set()
    for kw, text in (({'cout': -1}, "op 0 input channels outside 1 .. the destination tensor's channels"),
                     ({'cout': 9}, "op 0 input channels outside 1 .. the destination tensor's channels"),
                     ({'k': 2, 'cout': 16}, "op 0 input channels outside 1 .. the destination tensor's channels"),
                     ({'k': 2, 'cout': 6}, 'op 0 reorganised input channels not a multiple of 4'),
                     ({'k': 2, 'cout': 1}, 'op 0 reorganised input channels not a multiple of 4')):
        net, tensors, ops = V.network()
        _with_input(**kw)(net, tensors, ops)
        rc, msg = V.create(net, tensors, ops)
        assert rc == -1 and msg == 'yv7_plan_create: ' + text, (kw, rc, msg)
        seen.add(msg)
    assert len(seen) == 2
    for kw in ({'cout': 1}, {'cout': 5}, {'cout': 8}, {'k': 2, 'cout': 4}, {'k': 2, 'cout': 8}, {'cout': 0}):
        net, tensors, ops = V.network()
        _with_input(**kw)(net, tensors, ops)
        rc, msg = V.create(net, tensors, ops)
        assert rc not in (-1, -4) and (rc == 0 or not msg.startswith('yv7_plan_create:')), (kw, rc, msg)


@pytest.mark.parametrize('cin,ok', [(1, True), (2, True), (4, True), (5, False), (0, False), (12, False)])
def test_plan_create_stem_channel_counts(cin, ok):
    """A 32 / 64 STEM op takes the image's 1 .. 4 channels (12 belongs to the 64 / 128 ReOrg stem alone)."""
    net, tensors, ops = V.network()
    tensors[1][0] = 64
    ops.insert(1, V.op(kind=L.OP_STEM, cin=cin, cout=32, cout2=64, s=1, k=3, dst=1, w_off=0, b_off=0, w2_off=0,
                       b2_off=0))
    net['nbytes'] = V.NBYTES
    rc, msg = V.create(net, tensors, ops)
    if ok:   # (its weights: 32 x 64 and 64 x 320 halves; the blob must hold them)
        assert 'unsupported stem op' not in msg
    else:
        assert rc == -1 and 'unsupported stem op' in msg, (rc, msg)
