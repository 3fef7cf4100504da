"""yolov7-e6 / -d6 / -e6e on the CPU side: the generated cfgs, the DownC and Shortcut mirrors, the graph
compiler's DownC decomposition and ADD op, the descriptor validation of the ABI 5 fields, and the tests' own
CPU reference (tests/family_ref.py) against the oracle.

Reference: cfg/deploy|training/yolov7-{e6,d6,e6e}.yaml, models/common.py:80-86 (Shortcut), 181-192 (DownC),
models/yolo.py:747-787 (parse_model's channel rules for the two).
"""
import collections
import copy
import hashlib
import json
import os

import pytest
import torch

from family_nets import MINI_E6E, fresh
from yv7 import _lib as L
from yv7.graph import compile_model

REF_CFG = '/root/reference/cfg'
NAMES = ('yolov7-e6', 'yolov7-d6', 'yolov7-e6e')
# layers, len(save), parameters of the unfused model — taken once from the reference YAMLs
PINNED = {'yolov7-e6': (141, 90, 97246652), 'yolov7-d6': (163, 107, 133810044),
          'yolov7-e6e': (262, 185, 151757244), 'yolov7-e6-train': (145, 98, 111898292),
          'yolov7-d6-train': (167, 115, 154709364), 'yolov7-e6e-train': (266, 193, 166408884)}
DOWNC = {'yolov7-e6': 8, 'yolov7-d6': 8, 'yolov7-e6e': 8}
SHORTCUTS = {'yolov7-e6': 0, 'yolov7-d6': 0, 'yolov7-e6e': 11}


@pytest.fixture(scope='module')
def models():
    """name -> fused Model with its constructor's weights (structure tests need no trained values)."""
    from models.yolo import Model
    return {n: Model(n).fuse() for n in NAMES}


@pytest.mark.parametrize('name', sorted(PINNED))
def test_generated_cfg_equals_reference_yaml(name):
    """Key by key what yaml.safe_load gives for the reference file (where the reference is present), and the
    model it builds: layer count, save list, strides and parameter count."""
    from models.yolo import Model
    from yv7.arch import get_cfg
    cfg = get_cfg(name)
    train = name.endswith('-train')
    path = os.path.join(REF_CFG, 'training' if train else 'deploy', name[:-6] + '.yaml' if train else name + '.yaml')
    if os.path.exists(path):
        import yaml
        with open(path) as f:
            ref = yaml.safe_load(f)
        assert list(cfg) == list(ref)
        for k in ref:
            assert cfg[k] == ref[k], k
    m = Model(name)
    assert m.yaml['head'][-1][2] == ('IAuxDetect' if train else 'Detect')
    assert (len(m.model), len(m.save), sum(p.numel() for p in m.parameters())) == PINNED[name]
    assert m.stride.tolist() == [8.0, 16.0, 32.0, 64.0]


def test_yolov7x_stays_unregistered():
    from yv7.arch import get_cfg
    with pytest.raises(KeyError):
        get_cfg('yolov7x')


def test_family_ref_matches_oracle_bitwise_in_float64():
    """The restatement over the product's modules == the oracle's over the cfg dict and state_dict, to the
    last bit in float64 (same folds, same op order), and in fp32."""
    import family_ref
    from helpers import fresh_model, frames, oracle_net
    from oracle import yolo_ref
    net, fused = oracle_net('yolov7-tiny')
    m = fresh_model('yolov7-tiny')
    x = frames(2, 64, 64, seed=11)
    z64, xs64 = yolo_ref.forward64(net, fused, x)
    gz, gxs = family_ref.forward(m, x, torch.float64)
    assert gz.dtype == torch.float64 and torch.equal(gz, z64)
    assert all(torch.equal(a, b) for a, b in zip(gxs, xs64))
    z32, _ = yolo_ref.forward(net, fused, x)
    assert torch.equal(family_ref.forward(m, x)[0], z32)


# Instance attribute trees the reference's constructors create (tests/test_checkpoint.py REF_TREES'
# format: plain attributes, submodules, parameters, buffers): Shortcut common.py:81-83, DownC common.py:183-189.
REF_TREES = {'Shortcut': ({'d'}, set(), set(), set()),
             'DownC': (set(), {'cv1', 'cv2', 'cv3', 'mp'}, set(), set())}


def test_downc_shortcut_attribute_trees_match_reference():
    from models.yolo import Model
    m = Model(copy.deepcopy(MINI_E6E))
    seen = set()
    for mod in m.model:
        cls = type(mod).__name__
        if cls not in REF_TREES:
            continue
        plain = {k for k in vars(mod) if not k.startswith('_') and k != 'training'} - {'i', 'f', 'type', 'np'}
        assert (plain, set(mod._modules), set(mod._parameters), set(mod._buffers)) == REF_TREES[cls], cls
        seen.add(cls)
    assert seen == set(REF_TREES)
    d = m.model[2]
    c = [(x.conv.in_channels, x.conv.out_channels, x.conv.kernel_size[0], x.conv.stride[0]) for x in (d.cv1, d.cv2, d.cv3)]
    assert c == [(80, 80, 1, 1), (80, 80, 3, 2), (80, 80, 1, 1)]   # c_ = c1, c2 // 2 each (common.py:185-188)
    assert (d.mp.kernel_size, d.mp.stride) == (2, 2) and m.model[15].d == 1
    assert m.stride.tolist() == [4.0, 8.0]


def test_pickled_mini_e6e_roundtrips_through_attempt_load(tmp_path):
    """The reference's checkpoint format (train.py:465-472: the whole Model pickled in fp16) with DownC and
    Shortcut layers loads, fuses, and packs the same plan as building the model from the state_dict."""
    from models.common import Conv, DownC, Shortcut
    from models.experimental import attempt_load
    from models.yolo import Model
    src = fresh(('mini',), fuse=False)
    sd16 = {k: (v.half().float() if v.is_floating_point() else v) for k, v in src.state_dict().items()}
    m = src.half()
    del m._plans
    path = tmp_path / 'mini-e6e.pt'
    torch.save({'epoch': -1, 'model': m, 'ema': None}, path)
    got = attempt_load(str(path), map_location='cpu')
    assert isinstance(got, Model) and not got.training and next(got.parameters()).dtype == torch.float32
    assert sum(isinstance(x, DownC) for x in got.model) == 2 and sum(isinstance(x, Shortcut) for x in got.model) == 2
    assert not any(hasattr(x, 'bn') for x in got.modules() if type(x) is Conv)
    direct = Model(copy.deepcopy(MINI_E6E))
    direct.load_state_dict(sd16)
    direct = direct.float().fuse().eval()
    for dt in (L.DT_F32, L.DT_F16):
        a, b = compile_model(got, dt), compile_model(direct, dt)
        assert [o['kind'] for o in a.ops] == [o['kind'] for o in b.ops]
        assert torch.equal(a.weight_blob(), b.weight_blob())


@pytest.mark.parametrize('fuse', ['default', 'off', 'all'])
@pytest.mark.parametrize('dtype', [L.DT_F16, L.DT_F32], ids=['fp16', 'fp32'])
@pytest.mark.parametrize('name', NAMES)
def test_graph_structure(models, name, dtype, monkeypatch, fuse):
    """No COPY; every DownC is cv1, cv2 and (MAXPOOL + cv3 | one pooled cv3 where _fold_pools' conditions hold:
    fp16, cin % 64 == 0, cin <= 512) writing the two halves of one slice; every Shortcut is an ADD or the
    residual of a conv: none folded with YV7_NO_RESFUSE=1 or in fp32 plans, all of e6e's with YV7_RESFUSE=1."""
    from models.common import DownC
    from yv7.graph import RESFUSE_SHAPES
    from yv7.runtime import op_descs
    monkeypatch.delenv('YV7_NO_RESFUSE', raising=False)
    monkeypatch.delenv('YV7_RESFUSE', raising=False)
    if fuse != 'default':
        monkeypatch.setenv('YV7_NO_RESFUSE' if fuse == 'off' else 'YV7_RESFUSE', '1')
    m = models[name]
    g = compile_model(m, dtype)
    kinds = collections.Counter(o['kind'] for o in g.ops)
    assert kinds[L.OP_COPY] == 0
    res = [o for o in g.ops if o['kind'] == L.OP_CONV and o.get('src2', -1) >= 0]
    assert kinds[L.OP_ADD] + len(res) == SHORTCUTS[name]
    if fuse == 'off' or dtype == L.DT_F32:
        assert not res
    elif fuse == 'all':
        assert len(res) == SHORTCUTS[name]
    else:   # the measured rule (yv7.graph.RESFUSE_SHAPES)
        assert all((o['cout'], g.tensors[o['dst']][1]) in RESFUSE_SHAPES for o in res)
        assert not any((o['cout'], g.tensors[o['dst']][1]) in RESFUSE_SHAPES for o in g.ops if o['kind'] == L.OP_ADD)
    sc = {x.i: x for x in m.model if type(x).__name__ == 'Shortcut'}
    for o in res:   # a plain conv that closes a block, writing the Shortcut's slice; its own layer's tensor is gone
        assert 'merged' not in o and not o.get('pool') and o.get('wfmt', 0) == L.WFMT_PLAN and len(o['layers']) == 1
        lay = o['layers'][0][0]
        assert lay not in g.layer_tensor and lay + 1 in sc
        assert g.layer_tensor[lay + 1] == (o['dst'], o['dst_coff'], o['cout'])
        other = lay + 1 + sc[lay + 1].f[1]
        assert g.layer_tensor[other] == (o['src2'], o['src2_coff'], o['cout'])
        assert (o['src2'], o['src2_coff']) != (o['dst'], o['dst_coff'])
        assert g.tensors[o['src2']][1] == g.tensors[o['dst']][1]
    used = {o.get(k, -1) for o in g.ops for k in ('src', 'src2', 'dst')}
    assert max(used) == len(g.tensors) - 1
    downc = [x for x in m.model if isinstance(x, DownC)]
    assert len(downc) == DOWNC[name]
    by_tag = {tuple(t): o for o in g.ops if o['kind'] == L.OP_CONV for t in o['layers']}
    pooled = 0
    for d in downc:
        cv1, cv2, cv3 = (by_tag[(d.i, j)] for j in (1, 2, 3))
        cin = d.cv1.conv.in_channels
        assert cv2['src'] == cv1['dst'] and (cv2['k'], cv2['s']) == (3, 2)
        assert cv3['dst'] == cv2['dst'] and cv3['dst_coff'] == cv2['dst_coff'] + cv2['cout']
        fold = dtype == L.DT_F16 and cin % 64 == 0 and cin <= 512
        assert (cv3.get('pool', 0) == 2) == fold, (d.i, cin)
        if fold:
            assert (cv3['src'], cv3['src_coff'], cv3['s']) == (cv1['src'], cv1['src_coff'], 2)
            pooled += 1
        else:
            mp = [o for o in g.ops if o['kind'] == L.OP_MAXPOOL and o['dst'] == cv3['src']]
            assert len(mp) == 1 and (mp[0]['src'], mp[0]['src_coff'], mp[0]['k'], mp[0]['s']) == \
                (cv1['src'], cv1['src_coff'], 2, 2)
    assert sum(1 for o in g.ops if o.get('pool', 0) == 2) == pooled
    for o, d in zip(g.ops, op_descs(g)):
        if o['kind'] == L.OP_ADD:
            ts = [g.tensors[t] for t in (o['src'], o['src2'], o['dst'])]
            assert len({t[1] for t in ts}) == 1 and d.src2 == o['src2'] and d.src2_coff == o['src2_coff']
            assert g.layer_tensor[o['layer']] == (o['dst'], o['dst_coff'], o['cout'])
        elif o in res:
            assert d.src2 == o['src2'] and d.src2_coff == o['src2_coff']
        else:
            assert d.src2 == -1 and d.src2_coff == 0
    if name == 'yolov7-e6e':   # the auxiliary branch of the training twin is dropped: the same ops
        from models.yolo import Model
        t = compile_model(Model('yolov7-e6e-train').fuse(), dtype)
        assert [(o['kind'], o.get('cin'), o['cout']) for o in t.ops] == [(o['kind'], o.get('cin'), o['cout']) for o in g.ops]


def _fold_count(cfg, monkeypatch, dtype=L.DT_F16):
    from models.yolo import Model
    monkeypatch.setenv('YV7_RESFUSE', '1')
    monkeypatch.delenv('YV7_NO_RESFUSE', raising=False)
    g = compile_model(Model(copy.deepcopy(cfg)).fuse(), dtype)
    return g, sum(1 for o in g.ops if o['kind'] == L.OP_CONV and 'src2' in o), sum(o['kind'] == L.OP_ADD for o in g.ops)


def test_fold_shortcuts_conditions(monkeypatch):
    """The fold applies only where the ADD is the conv output's sole reader and the conv is plain; the conv then
    takes the OTHER operand as residual, never merges with a sibling, and the pass precedes the merges."""
    from models.yolo import Model
    g, nres, nadd = _fold_count(MINI_E6E, monkeypatch)
    assert (nres, nadd) == (2, 0)
    assert _fold_count(MINI_E6E, monkeypatch, L.DT_F32)[1:] == (0, 2)
    # layer 30 reads layer 14 beside the Shortcut (15): conv 14 has two readers and keeps its ADD; conv 8, the
    # ADD's other operand, runs before conv 14 has written its residual, so it cannot take it either.  The new
    # Shortcut 31 = conv 30 + layer 15 folds into conv 30 with layer 15 as the residual.
    cfg = copy.deepcopy(MINI_E6E)
    cfg['backbone'] += [[14, 1, 'Conv', [160, 1, 1]], [[30, 15], 1, 'Shortcut', [1]]]
    cfg['head'] = [[[31, 29], 1, 'Detect', ['nc', 'anchors']]]
    g, nres, nadd = _fold_count(cfg, monkeypatch)
    by = {o['layers'][0][0]: o for o in g.ops if o['kind'] == L.OP_CONV and 'src2' in o}
    assert set(by) == {28, 30} and nadd == 1
    assert (by[30]['src2'], by[30]['src2_coff']) == g.layer_tensor[15][:2]
    assert (by[30]['dst'], by[30]['dst_coff']) == g.layer_tensor[31][:2] and 30 not in g.layer_tensor
    # layer 30 reads the concat (13) that conv 14 reads, with conv 14's geometry: unfolded the two are siblings and
    # merge into one GEMM; the fold runs first and a conv that carries a residual never merges
    cfg['backbone'][30] = [13, 1, 'Conv', [160, 1, 1]]
    g, nres, nadd = _fold_count(cfg, monkeypatch)
    assert (nres, nadd) == (3, 0) and not any('merged' in o for o in g.ops if 'src2' in o)
    monkeypatch.delenv('YV7_RESFUSE')
    monkeypatch.setenv('YV7_NO_RESFUSE', '1')
    g = compile_model(Model(copy.deepcopy(cfg)).fuse(), L.DT_F16)
    assert any('merged' in o and {t[0] for t in o['layers']} == {14, 30} for o in g.ops)
    assert not any('src2' in o for o in g.ops if o['kind'] == L.OP_CONV)


@pytest.mark.parametrize('key', [('mini',), ('add', 48), ('res', 64)], ids=['mini', 'add48', 'res64'])
def test_plan_semantics_of_downc_and_shortcut(key, monkeypatch):
    """The compiled plans, executed op by op on the CPU (tests/plan_interp.py): the fp32 plan (DownC decomposed,
    Shortcut as ADD) reproduces family_ref's z to test_graph.py::test_plan_semantics_vs_oracle's tolerance, and the
    fp16 plan computes the same bits whether its Shortcuts run as ADDs or as the residual of a conv (default rule,
    all folded, none folded): a folded conv has no sibling in these nets, so no summation order changes.  add_net
    and res_net put the ADD / the residual at non-zero channel offsets of tensors of different widths."""
    import family_ref
    import plan_interp
    from helpers import frames
    m = fresh(key)
    x = frames(2, 32, 32)
    shortcuts = sum(type(l).__name__ == 'Shortcut' for l in m.model)
    monkeypatch.delenv('YV7_NO_RESFUSE', raising=False)
    monkeypatch.delenv('YV7_RESFUSE', raising=False)
    with torch.no_grad():
        torch.testing.assert_close(plan_interp.run(compile_model(m, L.DT_F32), x), family_ref.forward(m, x)[0],
                                   rtol=1e-4, atol=1e-3)
        split, zs = [], []
        for knob in (None, 'YV7_RESFUSE', 'YV7_NO_RESFUSE'):
            if knob:
                monkeypatch.setenv(knob, '1')
            g = compile_model(m, L.DT_F16)
            if knob:
                monkeypatch.delenv(knob)
            split.append((sum(o['kind'] == L.OP_CONV and 'src2' in o for o in g.ops),
                          sum(o['kind'] == L.OP_ADD for o in g.ops)))
            zs.append(plan_interp.run(g, x))
    assert all(r + a == shortcuts for r, a in split) and split[2][0] == 0
    if key == ('mini',):
        assert split == [(1, 1), (2, 0), (0, 2)]
    assert torch.equal(zs[0], zs[1]) and torch.equal(zs[0], zs[2])


def test_shortcut_of_unequal_inputs_is_rejected():
    from models.yolo import Model
    cfg = copy.deepcopy(MINI_E6E)
    cfg['backbone'][15] = [[-1, 2], 1, 'Shortcut', [1]]   # 160 channels at stride 4 + layer 2: fine
    compile_model(Model(copy.deepcopy(cfg)).fuse(), L.DT_F16)
    cfg['backbone'][15] = [[-1, 1], 1, 'Shortcut', [1]]   # + layer 1: 80 channels at stride 2
    with pytest.raises(ValueError, match='Shortcut'):
        compile_model(Model(cfg).fuse(), L.DT_F16)


# sha256 over the op dicts (src2 / src2_coff left out) and tensors of compile_model, computed on the commit
# before DownC / Shortcut / ABI 5: the existing models' plans did not move
PARENT_OPS = {('yolov7', L.DT_F16): (86, 'cb7c27aaa595d87b'), ('yolov7', L.DT_F32): (92, '1ff0a7186b2e6a9b'),
              ('yolov7-tiny', L.DT_F16): (57, 'd91d43008f269d23'), ('yolov7-tiny', L.DT_F32): (59, 'd4d5484bb2a9ddba'),
              ('yolov7-w6', L.DT_F16): (100, '8badeff10c920e55'), ('yolov7-w6', L.DT_F32): (102, '01ea0b1e67300e38')}


@pytest.mark.parametrize('name', ['yolov7', 'yolov7-tiny', 'yolov7-w6'])
def test_existing_models_compile_to_the_parent_op_lists(name):
    from models.yolo import Model
    from yv7.runtime import op_descs
    m = Model(name).fuse()
    for dt in (L.DT_F16, L.DT_F32):
        g = compile_model(m, dt)
        ops = [sorted((k, v) for k, v in o.items() if k not in ('src2', 'src2_coff')) for o in g.ops]
        h = hashlib.sha256(json.dumps([ops, g.tensors], default=list).encode()).hexdigest()[:16]
        assert (len(g.ops), h) == PARENT_OPS[(name, dt)]
        assert all(d.src2 == -1 and d.src2_coff == 0 for d in op_descs(g))


# ---- validate_net's rejections of the ABI 5 fields (the harness of tests/test_plan_validate.py)

def _add_net():
    from test_plan_validate import network, op
    net, tensors, ops = network()
    tensors += [[16, 0], [16, 0]]
    ops.insert(2, op(kind=L.OP_ADD, src=1, src2=2, dst=3, cout=16))
    return net, tensors, ops


def test_descriptor_with_add_passes_validation():
    from test_plan_validate import create
    rc, msg = create(*_add_net())
    assert rc not in (-1, -4), (rc, msg)
    assert rc == 0 or not msg.startswith('yv7_plan_create:'), (rc, msg)


def test_descriptor_with_residual_conv_passes_validation():
    from test_plan_validate import create
    net, tensors, ops = _add_net()
    ops[1].src2 = 2   # the 16-channel conv takes tensor 2 as its residual
    rc, msg = create(net, tensors, ops)
    assert rc not in (-1, -4), (rc, msg)
    assert rc == 0 or not msg.startswith('yv7_plan_create:'), (rc, msg)


def a_tensor(net, tensors, ops): ops[2].src2 = 9
def a_vector(net, tensors, ops): ops[2].cout = 12
def a_slice(net, tensors, ops): ops[2].src2_coff = 8
def a_first_slice(net, tensors, ops): ops[2].src_coff = 8
def a_shift(net, tensors, ops): tensors[2][1], net['max_shift'] = 1, 1
def a_overlap(net, tensors, ops): ops[2].dst = 2
def a_residual(net, tensors, ops): ops[1].src2 = 1
def r_pool(net, tensors, ops): ops[1].src2, ops[1].pool = 2, 2
def r_fp8(net, tensors, ops): ops[1].src2, ops[1].wfmt, ops[1].xscale = 2, L.WFMT_FP8, 1.0
def r_dtype(net, tensors, ops): ops[1].src2, net['dtype'] = 2, L.DT_F32
def r_tensor(net, tensors, ops): ops[1].src2 = 9
def r_negative(net, tensors, ops): ops[1].src2 = -2
def r_slice(net, tensors, ops): ops[1].src2, ops[1].src2_coff = 2, 8
def r_shift(net, tensors, ops): ops[1].src2, tensors[2][1], net['max_shift'] = 2, 1, 1
def a_stray(net, tensors, ops): ops[3].src2 = 0
def a_kind(net, tensors, ops): ops[2].kind = 8


ADD_CASES = [(a_tensor, 'op 2 bad second-operand tensor id'), (a_vector, 'op 2 add channels not a multiple of the vector'),
             (a_slice, 'op 2 second-operand channel slice out of range'), (a_first_slice, 'op 2 channel slice out of range'),
             (a_shift, 'op 2 add operands and result differ in resolution'), (a_overlap, 'op 2 add result overlaps an operand'),
             (a_residual, 'op 1 residual overlaps the result'), (a_stray, 'op 3 takes no second operand'),
             (r_pool, 'op 1 residual needs an fp16 plan'), (r_fp8, 'op 1 residual needs an fp16 plan'),
             (r_dtype, 'op 1 residual needs an fp16 plan'), (r_tensor, 'op 1 bad residual tensor id'),
             (r_negative, 'op 1 bad residual tensor id'), (r_slice, 'op 1 residual channel slice out of range'),
             (r_shift, 'op 1 residual and result differ in resolution'),
             (a_kind, 'op 2 unknown op kind')]


@pytest.mark.parametrize('mutate,want', ADD_CASES, ids=[m.__name__[2:] for m, _ in ADD_CASES])
def test_rejected_add_descriptor(mutate, want):
    from test_plan_validate import create
    net, tensors, ops = _add_net()
    mutate(net, tensors, ops)
    rc, msg = create(net, tensors, ops)
    assert rc == -1 and want in msg, (rc, msg)


def test_opdesc_defaults_to_no_second_operand():
    assert L.OpDesc().src2 == -1 and L.OpDesc(kind=L.OP_CONV, src=3).src2 == -1 and L.OpDesc(src2=4).src2 == 4
    assert L.ABI_VERSION == 5 and L.OP_ADD == 7
