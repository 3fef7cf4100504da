"""yv7_plan_create's descriptor validation (csrc/plan_create.cpp validate_net): every rejection's code and
message, on a minimal fp16 network — INPUT -> t0, CONV 3x3 t0 -> t1, DETECT on t1.  The validation runs
before any device is touched, so these cases need no GPU: each mutates one field of the valid descriptor
and expects YV7_E_ARG with that rejection's message.  (The null-argument and ABI-version cases are in
test_abi.py.)"""
import ctypes

import pytest

from yv7 import _lib as L

NBYTES = 12544   # conv w 32 x 128 fp16 at 0, bias at 8192; detect w 32 x 64 fp16 at 8256, bias at 12352


def op(**kw):
    d = dict(k=1, s=1)
    d.update(kw)
    return L.OpDesc(**d)


def network():
    """(net fields, tensors [[channels, shift]], ops) of the valid descriptor."""
    net = dict(dtype=L.DT_F16, nl=1, na=1, no=6, max_shift=0, nbytes=NBYTES)
    tensors = [[8, 0], [16, 0]]
    ops = [op(kind=L.OP_INPUT, dst=0),
           op(kind=L.OP_CONV, src=0, cin=8, dst=1, cout=16, k=3, s=1, pad=1, w_off=0, b_off=8192),
           op(kind=L.OP_DETECT, src=1, cin=16, cout=6, k=1, level=0, w_off=8256, b_off=12352)]
    return net, tensors, ops


def create(net, tensors, ops):
    """yv7_plan_create on the descriptor -> (rc, message); a plan that was created is destroyed."""
    lib = L.lib()
    ts = (L.TensorDesc * len(tensors))(*[L.TensorDesc(c, s) for c, s in tensors])
    os_ = (L.OpDesc * max(len(ops), 1))(*ops)
    stride = (ctypes.c_float * 1)(8.0)
    anchors = (ctypes.c_float * 8)(*[10.0] * 8)
    d = L.NetDesc(L.ABI_VERSION, net['dtype'], len(tensors), ts, net.get('n_ops', len(ops)), os_, net['nl'], net['na'],
                  net['no'], stride, anchors, net['max_shift'])
    blob = ctypes.create_string_buffer(NBYTES)
    h = ctypes.c_void_p()
    rc = lib.yv7_plan_create(ctypes.byref(d), ctypes.cast(blob, ctypes.c_void_p), net['nbytes'], 0, ctypes.byref(h))
    msg = lib.yv7_last_error().decode() if rc else ''
    if rc == 0:
        lib.yv7_plan_destroy(h)
    return rc, msg


def test_valid_descriptor_passes_validation():
    """Not an argument / ABI error: 0 with a GPU (the plan is destroyed), the HIP error of the first device
    call without one."""
    rc, msg = create(*network())
    assert rc not in (-1, -4), (rc, msg)
    assert rc == 0 or not msg.startswith('yv7_plan_create:'), (rc, msg)


def _stem(**kw):
    return op(kind=L.OP_STEM, cin=3, cout=32, cout2=64, s=1, k=3, dst=1, **kw)


def m_dtype(net, tensors, ops): net['dtype'] = 2
def m_empty(net, tensors, ops): net['n_ops'] = 0
def m_head(net, tensors, ops): net['na'] = 5
def m_channels(net, tensors, ops): tensors[1][0] = 12
def m_tensor_id(net, tensors, ops): ops[1].src = 7
def m_vector(net, tensors, ops): ops[1].cin = 4
def m_pool(net, tensors, ops): ops[1].pool = 2
def m_fp8(net, tensors, ops): ops[1].wfmt, ops[1].xscale = L.WFMT_FP8, 1.0
def m_blob(net, tensors, ops): net['nbytes'] = 12352
def m_window(net, tensors, ops): ops[1].pad = 2
def m_detect(net, tensors, ops): ops[2].cout = 12
def m_stem(net, tensors, ops): ops.insert(1, _stem())   # 64 output channels into the 16-channel t1
def m_slice(net, tensors, ops): ops[1].dst_coff = 8


def m_stem_blob(net, tensors, ops):
    tensors[1][0] = 64   # the stem now fits t1 (stem_supported: 3 -> 32 -> 64), its second conv's weights do not
    ops.insert(1, _stem(w2_off=1 << 20))


def m_pool_slice(net, tensors, ops):
    ops.insert(2, op(kind=L.OP_MAXPOOL, src=1, dst=1, dst_coff=8, cout=16))


CASES = [(m_dtype, 'bad dtype'), (m_empty, 'empty network'), (m_head, 'unsupported head geometry'),
         (m_channels, 'tensor 1 has bad channels/shift'), (m_tensor_id, 'op 1 bad tensor id'),
         (m_vector, 'not a multiple of the vector'), (m_pool, 'bad pooled conv'), (m_fp8, 'bad fp8 conv'),
         (m_blob, 'op 2 weight range outside blob'), (m_window, 'window reaches past'),
         (m_detect, 'bad detect op'), (m_stem, 'unsupported stem op'),
         (m_stem_blob, 'stem weight range outside blob'), (m_slice, 'op 1 channel slice out of range'),
         (m_pool_slice, 'op 2 channel slice out of range')]


@pytest.mark.parametrize('mutate,want', CASES, ids=[m.__name__[2:] for m, _ in CASES])
def test_rejected_descriptor(mutate, want):
    net, tensors, ops = network()
    mutate(net, tensors, ops)
    rc, msg = create(net, tensors, ops)
    assert rc == -1 and want in msg, (rc, msg)
