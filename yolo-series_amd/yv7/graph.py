"""Graph compiler: a models.yolo.Model -> the flat libyv7 plan (NHWC tensors, ops, packed weights).

Walks the parsed layer list the way forward_once does (models/yolo.py:601-631) and emits one op per
kernel launch:
  Conv / RepConv           -> CONV (BN / RepVGG branches folded in fp32 first, Model.fuse arithmetic)
  SPPCSPC                  -> 7 CONV + 3 MAXPOOL(5) cascaded (5, 5∘5 = 9, 5∘5∘5 = 13: max is associative and
                              the -inf padding clips identically), concats as channel slices (common.py:276-280)
  MP / SP                  -> MAXPOOL(k, k, 0) / MAXPOOL(k, s, k//2)
  nn.Upsample(x2 nearest)  -> UPSAMPLE
  DownC                    -> 3 CONV + MAXPOOL(2): cv1 into a private tensor, cv2 (3x3 stride 2) and mp + cv3 into the two
                              halves of the layer's output slice (common.py:181-192); fp16 plans fold mp + cv3 into
                              one pooled conv where _fold_pools' conditions hold
  Shortcut                 -> ADD (dst = src + src2, common.py:80-86); fp16 plans: folded into the conv that produces
                              one operand, as that conv's residual, where _fold_shortcuts' rule says it pays
  Concat                   -> nothing: producers write their channel slice of the concat tensor directly;
                              an input that already lives in another concat (or is the input image) gets a COPY
  ReOrg at layer 0         -> fused into the INPUT packing op (space-to-depth while converting NCHW -> NHWC);
                              fp16 plans of the w6 front end: ReOrg + its two convs as one STEM op
  Detect / IDetect / IAuxDetect -> one DETECT op per level (1x1 conv + bias + sigmoid + decode -> z)
Layers whose outputs never reach the head (IAuxDetect's auxiliary branch) are not emitted.
The image's channel count C is the model's (Model(cfg, ch=C), model.yaml['ch']): Graph.in_channels; the INPUT op
packs C (behind a ReOrg 4 C) channels, the fused 32 / 64 stem takes C <= 4 (_STEMS).

compile_model is the driver: layer shapes (_shapes), the front end (_front_end: INPUT op or fused STEM), concat
placement (_place_concats), one emitter per layer kind (_EMITTERS) over a shared _Lowering, then the op-list
rewrites at the end of this file (_fold_pools, _fold_shortcuts, _merge_siblings, _merge_sibling_tensors), then packing.

Weights: each conv's fused W [cout, cin, k, k] becomes [cout_pad32][k][k][cin_pad] (K padded to 64) in the
plan dtype, bias fp32 [cout_pad32]; every blob entry 256-byte aligned.
"""
from __future__ import annotations

import os
from collections import namedtuple
from dataclasses import dataclass, field

import torch
import torch.nn as nn

from models.common import MP, SP, SPPCSPC, Concat, Conv, DownC, ReOrg, RepConv, Shortcut
from models.yolo import Detect
from yv7 import _lib as L


@dataclass
class Graph:
    dtype: int
    tensors: list = field(default_factory=list)   # [channels, shift]
    ops: list = field(default_factory=list)       # dicts of OpDesc fields
    blobs: list = field(default_factory=list)     # (offset, uint8 tensor)
    nbytes: int = 0
    nl: int = 0
    na: int = 0
    no: int = 0
    stride: list = None
    anchor_grid: list = None
    max_shift: int = 0
    in_channels: int = 3                               # C of the [B,C,H,W] image (Model(cfg, ch=C))
    layer_tensor: dict = field(default_factory=dict)   # layer i -> (tensor, coff, channels) for debugging
    flops_per_pixel: float = 0.0                       # conv MACs*2 per input pixel (for roofline accounting)

    def add_tensor(self, channels, shift):
        self.tensors.append([channels, shift])
        return len(self.tensors) - 1

    def add_blob(self, t: torch.Tensor):
        b = t.contiguous().view(torch.uint8).reshape(-1).cpu()
        off = self.nbytes
        self.blobs.append((off, b))
        self.nbytes = (off + b.numel() + 255) // 256 * 256
        return off

    def weight_blob(self):
        out = torch.zeros(max(self.nbytes, 1), dtype=torch.uint8)
        for off, b in self.blobs:
            out[off:off + b.numel()] = b
        return out


def _vec(dtype):
    return 8 if dtype == L.DT_F16 else 4


def _rup(x, m):
    return (x + m - 1) // m * m


def _int(v):
    """A kernel size, stride or padding that torch keeps as an int or as a (h, w) pair."""
    return v if isinstance(v, int) else v[0]


def _act_code(act):
    if isinstance(act, nn.SiLU):
        return L.ACT_SILU
    if isinstance(act, nn.LeakyReLU):
        if abs(act.negative_slope - 0.1) > 1e-12:
            raise NotImplementedError('LeakyReLU slope other than 0.1')
        return L.ACT_LEAKY
    if isinstance(act, nn.Identity):
        return L.ACT_NONE
    raise NotImplementedError(f'activation {type(act).__name__}')


def _pad_rows(x: torch.Tensor, cols=None, dtype=torch.float32):
    """x [cout] or [cout, n] -> zero-padded [cout_pad32] or [cout_pad32, cols] of `dtype`."""
    out = torch.zeros([_rup(x.shape[0], 32)] + ([cols] if x.dim() == 2 else []), dtype=dtype)
    out[tuple(slice(n) for n in x.shape)] = x
    return out


def _pack_conv(g: Graph, w: torch.Tensor, b: torch.Tensor, cin_pad: int):
    """fp32 W [cout, cin, k, k] -> [cout_pad32][k*k*cin_pad -> K padded to 64] (plan dtype); bias fp32."""
    cout, cin, k, _ = w.shape
    tdt = torch.float16 if g.dtype == L.DT_F16 else torch.float32
    wk = w.permute(0, 2, 3, 1)  # [cout, k, k, cin]
    if cin_pad != cin:
        wk = torch.nn.functional.pad(wk, [0, cin_pad - cin])
    wp = _pad_rows(wk.reshape(cout, -1), _rup(k * k * cin_pad, 64))
    return g.add_blob(wp.to(tdt)), g.add_blob(_pad_rows(b))


def fp8_weight_scales(wk: torch.Tensor) -> torch.Tensor:
    """Per-output-channel e4m3 scales of a [cout, K] weight matrix: amax / 448 (1 for an all-zero row)."""
    amax = wk.abs().amax(1)
    return torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))


def _pack_conv_f8(g: Graph, w: torch.Tensor, b: torch.Tensor, cin_pad: int):
    """fp32 1x1 W [cout, cin, 1, 1] -> OCP e4m3 [cout_pad32][cin padded to 128] with per-output-channel
    scales wscale = amax / 448 (W ~ e4m3(W / wscale) * wscale, round to nearest even); bias fp32."""
    cout, cin = w.shape[:2]
    wk = w.reshape(cout, cin).float()
    ws = fp8_weight_scales(wk)
    q = (wk / ws[:, None]).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
    return (g.add_blob(_pad_rows(q, _rup(cin_pad, 128), torch.uint8)), g.add_blob(_pad_rows(b)),
            g.add_blob(_pad_rows(ws)))


def fp8_eligible(g: Graph, o: dict) -> bool:
    """CONV ops an fp8 plan runs in e4m3: 1x1 stride-1 convs of an fp16 plan (the Detect head stays fp16)."""
    return (g.dtype == L.DT_F16 and o['kind'] == L.OP_CONV and o['k'] == 1 and o['s'] == 1 and o['pad'] == 0
            and o['cout'] <= 1024 and 'src2' not in o)   # (a conv that carries a residual stays fp16)


# fp8 pays only on wide layers: measured per op on MI355X (bs32 640 yolov7, scripts/op_profile.py
# --dtype fp8 vs f16), cout >= 512 gains 1-41 us per layer (1024->1024 @40: 156 -> 114 us) while every
# cout <= 256 layer loses 3-82 us — their time is the SiLU epilogue and the extra quantize pass, not
# the MFMA, so the 2x fp8 MFMA rate cannot win it back.
FP8_MIN_COUT = 512


def fp8_candidates(g: Graph, min_cout: int = FP8_MIN_COUT):
    """Op indices of `g` that compile_model(..., fp8={index: xscale}) marks FP8 in an fp8 plan: the
    fp8-eligible ops with at least `min_cout` output channels (min_cout=0: every eligible op)."""
    return [i for i, o in enumerate(g.ops) if fp8_eligible(g, o) and o['cout'] >= min_cout]


def _pack(g: Graph, fp8: dict):
    """Pack the weights the convs carried through the rewrites, in op order; the ops of `fp8` in e4m3."""
    for idx, o in enumerate(g.ops):
        if '_w' in o:
            w, b = o.pop('_w'), o.pop('_b')
            if idx in fp8:
                if not fp8_eligible(g, o):
                    raise ValueError(f'op {idx} cannot run in fp8 (fp16 plans, 1x1 stride-1 convs only)')
                o['w_off'], o['b_off'], o['s_off'] = _pack_conv_f8(g, w, b, o['cin'])
                o['wfmt'], o['xscale'] = L.WFMT_FP8, float(fp8[idx])
            else:
                o['w_off'], o['b_off'] = _pack_conv(g, w, b, o['cin'])


def _sources(m):
    """The layers m reads, as absolute indices; -1 is the input image."""
    return [max(m.i + j, -1) if j < 0 else j for j in ([m.f] if isinstance(m.f, int) else m.f)]


def _conv2d(m):
    """The nn.Conv2d of a Conv or of a RepConv (deployed, or its 3x3 branch)."""
    return m.conv if isinstance(m, Conv) else (m.rbr_reparam if hasattr(m, 'rbr_reparam') else m.rbr_dense[0])


def _live_layers(layers, nl):
    """Layers whose output reaches the Detect head (drops IAuxDetect's auxiliary branch)."""
    need = [False] * len(layers)
    need[-1] = True
    for m in reversed(layers):
        if need[m.i]:
            for j in _sources(m)[:nl] if isinstance(m, Detect) else _sources(m):
                if j >= 0:
                    need[j] = True
    return need


def _shapes(layers, c_in):
    """layer -> output channels, layer -> spatial shift (log2 of the stride); -1 is the input image."""
    ch, shift = {-1: c_in}, {-1: 0}
    for m in layers:
        i = m.i
        prev = _sources(m)
        pc = [ch[j] for j in prev]
        ps = [shift[j] for j in prev]
        if isinstance(m, (Conv, RepConv)):
            ch[i], shift[i] = _conv2d(m).out_channels, ps[0] + (1 if _conv2d(m).stride[0] == 2 else 0)
        elif isinstance(m, SPPCSPC):
            ch[i], shift[i] = m.cv7.conv.out_channels, ps[0]
        elif isinstance(m, DownC):
            ch[i], shift[i] = m.cv2.conv.out_channels + m.cv3.conv.out_channels, ps[0] + 1
        elif isinstance(m, Shortcut):
            if len(prev) != 2 or pc[0] != pc[1] or ps[0] != ps[1]:
                raise ValueError(f'layer {i}: Shortcut needs two inputs of equal channels and resolution')
            ch[i], shift[i] = pc[0], ps[0]
        elif isinstance(m, MP):
            ch[i], shift[i] = pc[0], ps[0] + 1
        elif isinstance(m, SP):
            ch[i], shift[i] = pc[0], ps[0]
        elif isinstance(m, nn.Upsample):
            if m.mode != 'nearest' or float(m.scale_factor) != 2.0:
                raise NotImplementedError('only nn.Upsample(scale_factor=2, mode="nearest")')
            ch[i], shift[i] = pc[0], ps[0] - 1
        elif isinstance(m, ReOrg):
            if i != 0:
                raise NotImplementedError('ReOrg is supported as the first layer (fused into input packing)')
            ch[i], shift[i] = pc[0] * 4, ps[0] + 1
        elif isinstance(m, Concat):
            if len(set(ps)) != 1:
                raise ValueError(f'layer {i}: concat of different resolutions')
            ch[i], shift[i] = sum(pc), ps[0]
        elif isinstance(m, Detect):
            ch[i], shift[i] = 0, 0
        else:
            raise NotImplementedError(f'layer {i}: {type(m).__name__}')
    return ch, shift


# The front ends that run as one fused fp16 STEM op (csrc/stem.hip) straight from the image: [ReOrg ->] conv A
# (3x3, pad 1) -> conv B (3x3, stride 2, pad 1), every layer before B read only by its successor.  Per row:
# leading ReOrg; A's cin (the image's channels C where there is no ReOrg: Model(cfg, ch=C), any count the patch's
# four channel slots hold), cout, strides; B's cout; A's K pad per tap (None: cin itself, K = tap * C + ci; the w6
# row reads the 12-channel space-to-depth image with K = tap * 16 + ci).  Whatever matches no row (a ReOrg model
# with C != 3, any model with C > 4) lowers to INPUT + CONV ops.
_STEMS = ((False, (1, 2, 3, 4), 32, (1, 2), 64, None),  # yolov7 / yolov7-tiny, layers 0-1
          (True, (12,), 64, (1,), 128, 16))  # yolov7-w6, layers 0-2 (cfg/deploy/yolov7-w6.yaml:14-16, stem_reorg_kernel)
_Stem = namedtuple('_Stem', 'at cin kpad')   # the layer that carries the op (layers before it are folded into it)


def _stem_candidate(layers, dtype):
    """The row of _STEMS the first layers match, as a _Stem, or None (fp16 plans only)."""
    if dtype != L.DT_F16:
        return None
    for reorg, cins, cout, strides, cout2, kpad in _STEMS:
        at = 2 if reorg else 1
        if len(layers) < at + 2 or isinstance(layers[0], ReOrg) != reorg:
            continue
        la, lb = layers[at - 1], layers[at]
        if not (type(la) is Conv and type(lb) is Conv and all(m.f == -1 for m in layers[1:at + 1])):
            continue
        a, b = la.conv, lb.conv
        if not (a.in_channels in cins and a.out_channels == cout and a.kernel_size[0] == 3 and a.stride[0] in strides
                and a.padding[0] == 1 and b.out_channels == cout2 and b.kernel_size[0] == 3 and b.stride[0] == 2
                and b.padding[0] == 1 and a.groups == 1 and b.groups == 1 and _act_code(la.act) == _act_code(lb.act)):
            continue
        if any(j < at for m in layers[at + 1:] for j in _sources(m) if j >= 0):
            continue
        return _Stem(at, a.in_channels, kpad or a.in_channels)
    return None


# ---- lowering

@dataclass
class _Lowering:
    """What the emitters share: the graph under construction and where every layer's output lives."""
    g: Graph
    V: int                # channels per vector access of the plan dtype
    ch: dict              # layer -> channels (_shapes)
    shift: dict
    t_in: int             # the packed input image: tensor, channels
    in_c: int
    loc: dict = field(default_factory=dict)      # layer -> (tensor, coff)
    placed: set = field(default_factory=set)     # (layer, concat) pairs written in place (_place_concats)

    def src_of(self, j):
        return (self.t_in, 0, self.in_c) if j < 0 else (*self.loc[j], self.ch[j])

    def out_of(self, i):
        if i not in self.loc:
            self.loc[i] = (self.g.add_tensor(_rup(self.ch[i], self.V), self.shift[i]), 0)
        return self.loc[i]

    def conv(self, mod, src, dst, tag):
        """CONV for the Conv / RepConv `mod` from slice `src` to (tensor, offset) `dst`.  The weights are packed
        after the rewrites (_merge_siblings concatenates them), so they ride along unpacked; tag = (layer,
        cv index inside an SPPCSPC / DownC or None) names the reference conv(s) an op computes."""
        (ts, so, cs), (td, do) = src, dst
        w, b = mod.fused_weight_bias()
        c = _conv2d(mod)
        cin_pad = _rup(cs, self.V)
        if cin_pad != cs and self.g.tensors[ts][0] < so + cin_pad:
            raise ValueError('channel padding would read outside the source tensor')
        self.g.ops.append(dict(kind=L.OP_CONV, src=ts, src_coff=so, cin=cin_pad, dst=td, dst_coff=do, cout=w.shape[0],
                               k=c.kernel_size[0], s=c.stride[0], pad=c.padding[0], act=_act_code(mod.act), _w=w, _b=b,
                               layers=[tag]))

    def op(self, kind, src, dst, **kw):
        """A channel-preserving op (MAXPOOL, UPSAMPLE, ADD, COPY) from slice `src` to (tensor, offset) `dst`."""
        (ts, so, cs), (td, do) = src, dst
        self.g.ops.append(dict(kind=kind, src=ts, src_coff=so, dst=td, dst_coff=do, cout=cs, **kw))


def _front_end(g: Graph, layers, V, ch, shift, stem):
    """Tensor 0, the packed network input: written by the INPUT op (a ReOrg at layer 0 is fused into it), or an
    unused placeholder where the fused stem reads the image itself.  The INPUT op's cout is what the C side packs:
    the image's C channels, 4 C behind a ReOrg."""
    reorg0 = isinstance(layers[0], ReOrg)
    in_c = 4 * ch[-1] if reorg0 else ch[-1]
    if stem is not None:
        return _Lowering(g, V, ch, shift, g.add_tensor(V, g.max_shift), in_c)
    cx = _Lowering(g, V, ch, shift, g.add_tensor(_rup(in_c, V), 1 if reorg0 else 0), in_c)
    g.ops.append(dict(kind=L.OP_INPUT, src=-1, dst=cx.t_in, k=2 if reorg0 else 1, cout=in_c))
    if reorg0:
        cx.loc[0] = (cx.t_in, 0)
    return cx


def _place_concats(cx, layers, live):
    """Producers write straight into the concat tensor: every live Concat gets its tensor, and each input that has
    no place yet and can be written at its offset is placed there."""
    placeable = (Conv, RepConv, SPPCSPC, DownC, Shortcut, MP, SP, nn.Upsample)
    for m in layers:
        if isinstance(m, Concat) and live[m.i]:
            t = cx.g.add_tensor(_rup(cx.ch[m.i], cx.V), cx.shift[m.i])
            cx.loc[m.i] = (t, 0)
            off = 0
            for j in _sources(m):
                if j >= 0 and j not in cx.loc and isinstance(layers[j], placeable) and cx.ch[j] % cx.V == 0 and \
                        off % cx.V == 0:
                    cx.loc[j] = (t, off)
                    cx.placed.add((j, m.i))
                off += cx.ch[j]


def _emit_stem(cx, layers, stem):
    la, lb = layers[stem.at - 1], layers[stem.at]
    wa_off, ba_off = _pack_conv(cx.g, *la.fused_weight_bias(), stem.kpad)
    wb_off, bb_off = _pack_conv(cx.g, *lb.fused_weight_bias(), lb.conv.in_channels)
    td, do = cx.out_of(stem.at)
    cx.g.ops.insert(0, dict(kind=L.OP_STEM, src=-1, cin=stem.cin, cout=la.conv.out_channels, k=3, s=la.conv.stride[0],
                            pad=1, act=_act_code(la.act), w_off=wa_off, b_off=ba_off, dst=td, dst_coff=do,
                            cout2=lb.conv.out_channels, act2=_act_code(lb.act), w2_off=wb_off, b2_off=bb_off))


def _emit_conv(cx, m):
    c = _conv2d(m)
    if c.groups != 1 or c.dilation[0] != 1:
        raise NotImplementedError('grouped / dilated conv')
    cx.conv(m, cx.src_of(_sources(m)[0]), cx.out_of(m.i), (m.i, None))


def _emit_sppcspc(cx, m):
    g, V, i = cx.g, cx.V, m.i
    src = cx.src_of(_sources(m)[0])
    c_ = m.cv1.conv.out_channels
    t1, t3, cat1, t5, cat2 = (g.add_tensor(_rup(n * c_, V), cx.shift[i]) for n in (1, 1, 4, 1, 2))
    if c_ % V:
        raise NotImplementedError('SPPCSPC hidden width must be a multiple of the vector width')
    cx.conv(m.cv1, src, (t1, 0), (i, 1))
    cx.conv(m.cv3, (t1, 0, c_), (t3, 0), (i, 3))
    cx.conv(m.cv4, (t3, 0, c_), (cat1, 0), (i, 4))
    ks = [p.kernel_size for p in m.m]
    if ks == [5, 9, 13]:  # cascade: pool9 = pool5(pool5), pool13 = pool5(pool9)
        for q in range(3):
            cx.op(L.OP_MAXPOOL, (cat1, q * c_, c_), (cat1, (q + 1) * c_), k=5, s=1, pad=2)
    else:
        for q, k in enumerate(ks):
            cx.op(L.OP_MAXPOOL, (cat1, 0, c_), (cat1, (q + 1) * c_), k=k, s=1, pad=k // 2)
    cx.conv(m.cv5, (cat1, 0, 4 * c_), (t5, 0), (i, 5))
    cx.conv(m.cv6, (t5, 0, c_), (cat2, 0), (i, 6))
    cx.conv(m.cv2, src, (cat2, c_), (i, 2))
    cx.conv(m.cv7, (cat2, 0, 2 * c_), cx.out_of(i), (i, 7))


def _emit_downc(cx, m):
    i = m.i
    src = cx.src_of(_sources(m)[0])
    cs, c_, ch2 = src[2], m.cv1.conv.out_channels, m.cv2.conv.out_channels
    if _int(m.mp.kernel_size) != 2 or cs % cx.V or c_ % cx.V or ch2 % cx.V:
        raise NotImplementedError('DownC: k = 2 and widths that are multiples of the vector width only')
    td, do = cx.out_of(i)
    t1 = cx.g.add_tensor(c_, cx.shift[i] - 1)
    tp = cx.g.add_tensor(cs, cx.shift[i])
    cx.conv(m.cv1, src, (t1, 0), (i, 1))
    cx.conv(m.cv2, (t1, 0, c_), (td, do), (i, 2))
    cx.op(L.OP_MAXPOOL, src, (tp, 0), k=2, s=2, pad=0)
    cx.conv(m.cv3, (tp, 0, cs), (td, do + ch2), (i, 3))


def _emit_shortcut(cx, m):
    a, b = (cx.src_of(j) for j in _sources(m))
    if a[2] % cx.V:
        raise NotImplementedError('Shortcut width not a multiple of the vector width')
    cx.op(L.OP_ADD, a, cx.out_of(m.i), src2=b[0], src2_coff=b[1], layer=m.i)


def _emit_pool(cx, m):
    cx.op(L.OP_MAXPOOL, cx.src_of(_sources(m)[0]), cx.out_of(m.i), k=_int(m.m.kernel_size), s=_int(m.m.stride),
          pad=_int(m.m.padding), layer=m.i)


def _emit_concat(cx, m):
    """Nothing for the inputs placed in the concat tensor; a COPY for each of the others."""
    t, _ = cx.loc[m.i]
    off = 0
    for j in _sources(m):
        src = cx.src_of(j)
        if (j, m.i) not in cx.placed:
            if src[2] % cx.V or off % cx.V:
                raise NotImplementedError('concat slice not a multiple of the vector width')
            cx.op(L.OP_COPY, src, (t, off))
        off += src[2]


def _emit_detect(cx, m):
    for lvl, j in enumerate(_sources(m)[:m.nl]):
        ts, so, cs = cx.src_of(j)
        w, b = m.head_weights(lvl)
        w_off, b_off = _pack_conv(cx.g, w, b, _rup(cs, cx.V))
        cx.g.ops.append(dict(kind=L.OP_DETECT, src=ts, src_coff=so, cin=_rup(cs, cx.V), dst=-1, cout=w.shape[0],
                             k=1, s=1, pad=0, level=lvl, w_off=w_off, b_off=b_off))


# first match wins, in _shapes' order (Detect covers IDetect and IAuxDetect); a ReOrg (layer 0) emits nothing
_EMITTERS = (((Conv, RepConv), _emit_conv), (SPPCSPC, _emit_sppcspc), (DownC, _emit_downc), (Shortcut, _emit_shortcut),
             ((MP, SP), _emit_pool),
             (nn.Upsample, lambda cx, m: cx.op(L.OP_UPSAMPLE, cx.src_of(_sources(m)[0]), cx.out_of(m.i))),
             (ReOrg, lambda cx, m: None), (Concat, _emit_concat), (Detect, _emit_detect))


def compile_model(model, dtype: int, fp8=None) -> Graph:
    """fp8: {op index: activation scale} — those ops (fp8_candidates of the same model and dtype) are
    packed as YV7_WFMT_FP8 (e4m3 weights + scales); the op list is otherwise identical."""
    no_stem, no_poolfold, no_resfuse, resfuse_all, no_merge, no_tmerge = (
        os.environ.get(k) == '1' for k in ('YV7_NO_STEM', 'YV7_NO_POOLFOLD', 'YV7_NO_RESFUSE', 'YV7_RESFUSE',
                                           'YV7_NO_MERGE', 'YV7_NO_TMERGE'))
    f16 = dtype == L.DT_F16
    layers = list(model.model)
    det = layers[-1]
    if not isinstance(det, Detect):
        raise NotImplementedError('the last layer must be a Detect / IDetect / IAuxDetect head')
    g = Graph(dtype=dtype, nl=det.nl, na=det.na, no=det.no)
    g.stride = [float(s) for s in det.stride]
    g.anchor_grid = det.anchor_grid.detach().float().cpu().reshape(-1).tolist()
    live = _live_layers(layers, det.nl)
    ch, shift = _shapes(layers, model.yaml.get('ch', 3))
    g.max_shift = max(shift.values())
    g.in_channels = ch[-1]

    stem = None if no_stem else _stem_candidate(layers, dtype)
    cx = _front_end(g, layers, _vec(dtype), ch, shift, stem)
    _place_concats(cx, layers, live)
    for m in layers[stem.at if stem else 0:]:
        if not live[m.i]:
            continue
        if stem and m.i == stem.at:
            _emit_stem(cx, layers, stem)
        else:
            next(emit for kinds, emit in _EMITTERS if isinstance(m, kinds))(cx, m)

    folded = _fold_pools(g) if f16 and not no_poolfold else []
    if f16 and not no_resfuse:
        folded += _fold_shortcuts(g, cx.loc, every=resfuse_all)
    if not no_merge:
        _merge_siblings(g)
        if not no_tmerge:
            _merge_sibling_tensors(g, cx.loc)
    _pack(g, fp8 or {})
    g.layer_tensor = {i: (cx.loc[i][0], cx.loc[i][1], ch[i]) for i in cx.loc if i not in folded}
    return g


# ---- the op-list rewrites, and the one vocabulary in which they ask about data flow: a slice is (tensor, first
# channel, channels); _reads(o) and _writes(o) give the slices an op touches, _overlaps compares two, _touch finds
# the ops of a list that read or write one.  No pass compares channel offsets itself.  The passes that remove or
# join tensors keep `loc`, the lowering's layer -> (tensor, offset) map, in step.

def _reads(o):
    """The (tensor, first channel, channels) slices an op reads."""
    r = []
    if o.get('src', -1) >= 0:
        r.append((o['src'], o.get('src_coff', 0), o['cin'] if o['kind'] in (L.OP_CONV, L.OP_DETECT) else o['cout']))
    if o.get('src2', -1) >= 0:
        r.append((o['src2'], o['src2_coff'], o['cout']))
    return r


def _writes(o):
    """(tensor, first channel, channels) an op writes, or None (DETECT writes z)."""
    if o['kind'] == L.OP_DETECT:
        return None
    if o['kind'] == L.OP_STEM:
        return o['dst'], o['dst_coff'], o['cout2']
    return o['dst'], o.get('dst_coff', 0), o['cout']   # (INPUT names no offset: it writes tensor 0 whole)


def _overlaps(a, b):
    (t, lo, n), (t2, lo2, n2) = a, b
    return t == t2 and lo < lo2 + n2 and lo2 < lo + n


def _touch(ops, sl, reads=False, writes=False):
    """Indices into `ops` of the ops that read (reads=True) or write (writes=True) a slice overlapping `sl`."""
    return [j for j, o in enumerate(ops)
            if (reads and any(_overlaps(r, sl) for r in _reads(o)))
            or (writes and _writes(o) is not None and _overlaps(_writes(o), sl))]


def _whole(g, t):
    return t, 0, g.tensors[t][0]


def _fold_pools(g):
    """MP (2x2 / stride-2 max, models/common.py:30-36) whose output only feeds one 1x1 conv of <= 512 input
    channels (yolov7: `[-1, 1, MP, []], [-1, 1, Conv, [c, 1, 1]]`) -> that conv reads the MP's input with
    pool = 2, s = 2: the max is taken in the conv's operand loads and the pooled tensor never reaches
    HBM.  Returns the folded MP layers (their outputs no longer exist as tensors)."""
    folded = []
    i = 0
    while i < len(g.ops):
        mp = g.ops[i]
        if not (mp['kind'] == L.OP_MAXPOOL and mp['k'] == 2 and mp['s'] == 2 and mp['pad'] == 0):
            i += 1
            continue
        t = mp['dst']
        readers = _touch(g.ops, _whole(g, t), reads=True)
        c = g.ops[readers[0]] if readers else None
        if not (len(readers) == 1 and readers[0] > i and _touch(g.ops, _whole(g, t), writes=True) == [i] and
                c['kind'] == L.OP_CONV and '_w' in c and c['src'] == t and c['k'] == 1 and c['s'] == 1 and
                c['pad'] == 0 and c['src_coff'] == mp['dst_coff'] and c['cin'] == mp['cout'] and c['cin'] % 64 == 0 and
                c['cin'] <= 512):   # deep-K (1024) pairs run faster unfused (csrc/conv_f16.hip, pool dispatch)
            i += 1
            continue
        c.update(src=mp['src'], src_coff=mp['src_coff'], s=2, pool=2)
        folded.append(mp.get('layer'))
        del g.ops[i]
    return folded


# Shapes (output channels, log2 stride) whose Shortcut runs folded into its producer by default: those where the
# fused launch measured faster than conv + add by more than the run-to-run spread (yolov7-e6e
# 1280 x 1280 bs 8).  YV7_RESFUSE=1 folds every eligible Shortcut, YV7_NO_RESFUSE=1 none.
RESFUSE_SHAPES = frozenset({(160, 2), (160, 3), (480, 5), (640, 6), (1280, 6)})


def _residual_host(g, a, own, res):
    """Index of the conv that can produce ADD op a's operand slice `own` straight into the ADD's destination with
    the other operand `res` as its residual, or None."""
    dst = _writes(g.ops[a])
    writers = _touch(g.ops, own, writes=True)
    if len(writers) != 1 or _touch(g.ops, own, reads=True) != [a] or writers[0] > a:
        return None
    w = writers[0]
    c = g.ops[w]
    if not (c['kind'] == L.OP_CONV and '_w' in c and not c.get('pool') and 'src2' not in c and
            _writes(c) == own and c['dst_coff'] == 0 and g.tensors[c['dst']][0] == c['cout']):
        return None
    if _overlaps(res, dst) or _overlaps(own, res):
        return None
    # the residual is complete before the conv; between the conv and the ADD nothing touches the
    # destination
    if _touch(g.ops[w:a], res, writes=True):
        return None
    if _touch(g.ops[w + 1:a], dst, reads=True, writes=True):
        return None
    return w


def _fold_shortcuts(g, loc: dict, every=False):
    """ADD (Shortcut, models/common.py:80-86) whose one operand is the whole output of a plain CONV (not pooled,
    not a STEM; it runs before the sibling merges and such a conv never merges; fp8 never takes it) that nothing
    else reads -> that conv takes the other operand as its residual (src2) and writes the ADD's destination: the
    conv's epilogue adds it in fp32 and rounds once (csrc/conv_f16_ring.hip), the ADD and the conv's own output
    tensor disappear.  The residual must be complete before the conv runs and must not overlap the destination;
    nothing between the conv and the ADD may touch the destination (_residual_host).  Folds the ADDs whose shape
    is in RESFUSE_SHAPES, all eligible ones with `every`.  Returns the layers whose outputs no longer exist as
    tensors."""
    folded = []
    a = 0
    while a < len(g.ops):
        add = g.ops[a]
        if add['kind'] == L.OP_ADD and (every or (add['cout'], g.tensors[add['dst']][1]) in RESFUSE_SHAPES):
            first, second = _reads(add)
            w, res = _residual_host(g, a, first, second), second
            if w is None:
                w, res = _residual_host(g, a, second, first), first
            if w is not None:
                c = g.ops[w]
                dead = c['dst']
                c.update(dst=add['dst'], dst_coff=add['dst_coff'], src2=res[0], src2_coff=res[1])
                del g.ops[a]
                for lay, _ in c['layers']:
                    folded.append(lay)
                    loc.pop(lay, None)
                _drop_tensor(g, loc, dead)
                continue
        a += 1
    return folded


def _remap_tensors(g, loc: dict, f):
    """Rename tensors: f(tensor, offset) -> (tensor, offset) is applied to the source, residual and destination of
    every op and to every entry of loc.  An op that names no offset (INPUT) gains one only if it becomes non-zero."""
    for o in g.ops:
        for k in ('src', 'src2', 'dst'):
            if o.get(k, -1) >= 0:
                o[k], off = f(o[k], o.get(k + '_coff', 0))
                if off or k + '_coff' in o:
                    o[k + '_coff'] = off
    for lay, (t, off) in list(loc.items()):
        loc[lay] = f(t, off)


def _drop_tensor(g, loc: dict, t: int):
    """Remove tensor t, which no op touches any more (higher ids shift down in every op and in loc)."""
    assert not _touch(g.ops, _whole(g, t), reads=True, writes=True)
    _remap_tensors(g, loc, lambda u, off: (u - 1 if u > t else u, off))
    del g.tensors[t]


def _fuse_tensors(g, loc: dict, t1: int, t2: int):
    """Tensor t2 becomes channels [C1, C1 + C2) of tensor t1; t2's id is removed (higher ids shift down)
    in every op and in the layer -> (tensor, offset) map."""
    c1 = g.tensors[t1][0]
    g.tensors[t1][0] = c1 + g.tensors[t2][0]

    def f(u, off):
        if u == t2:
            u, off = t1, off + c1
        return (u - 1 if u > t2 else u), off

    _remap_tensors(g, loc, f)
    for o in g.ops:   # (from the first fuse on the INPUT op names its offset: plans are pinned key for key)
        if o['kind'] == L.OP_INPUT:
            o.setdefault('dst_coff', 0)
    del g.tensors[t2]


def _may_move_up(ops, i, j):
    """ops[j], a conv, may run at position i instead: nothing in between writes its input or reads / writes its
    output slice."""
    between, (src,) = ops[i + 1:j], _reads(ops[j])
    return not _touch(between, src, writes=True) and not _touch(between, _writes(ops[j]), reads=True, writes=True)


def _merge_scan(g, key, pair, loc=None):
    """The scan both sibling merges share.  For every plain CONV a (weights unpacked, no residual) and every later
    one b that agrees with it on `key` (the input slice and the geometry): where pair(a, b) names them (lo, hi) in
    output-channel order and b may move up to a's position, the two become one GEMM of N = cout_a + cout_b at a's
    position, weights and biases concatenated lo first.  The search for b ends where a's input is overwritten.
    With loc the two outputs are separate tensors, fused into [lo's | hi's] first, and a is tried again after a
    merge (its new tensor may have another sibling); without, the scan steps on."""
    i = 0
    while i < len(g.ops):
        merged = _plain_conv(g.ops[i]) and _merge_at(g, i, key, pair, loc)
        if not (merged and loc is not None):
            i += 1


def _plain_conv(o):
    return o['kind'] == L.OP_CONV and '_w' in o and 'src2' not in o


def _merge_at(g, i, key, pair, loc):
    """Merge a = g.ops[i] with its first later sibling that qualifies (_merge_scan); True if one did."""
    a = g.ops[i]
    for j in range(i + 1, len(g.ops)):
        b = g.ops[j]
        lo_hi = pair(a, b) if _plain_conv(b) and all(a.get(k) == b.get(k) for k in key) else None
        if lo_hi and _may_move_up(g.ops, i, j):
            lo, hi = lo_hi
            if loc is not None:
                _fuse_tensors(g, loc, lo['dst'], hi['dst'])
            m = dict(a)
            m.update(dst=lo['dst'], dst_coff=lo['dst_coff'], cout=lo['cout'] + hi['cout'],
                     _w=torch.cat([lo['_w'], hi['_w']], 0), _b=torch.cat([lo['_b'], hi['_b']], 0),
                     merged=(lo['cout'], hi['cout']), layers=lo['layers'] + hi['layers'])
            g.ops[i] = m
            del g.ops[j]
            return True
        if _touch([b], _reads(a)[0], writes=True):
            return False  # a's input is overwritten from here on
    return False


_SIBLING_KEY = ('src', 'src_coff', 'cin', 'k', 's', 'pad', 'act', 'pool')


def _merge_siblings(g):
    """Fold pairs of CONV ops that read the same input slice with the same geometry and activation and
    write adjacent channel slices of one tensor into a single GEMM with N = cout_a + cout_b.

    In every ELAN block the two 1x1 entry convs (e.g. yolov7.yaml:20-21 `[-1, 1, Conv, [64, 1, 1]]`,
    `[-2, 1, Conv, [64, 1, 1]]`) both read the previous layer and land side by side in the block's
    concat (`[[-1, -3, -5, -6], 1, Concat, [1]]` puts -5 and -6 next to each other): one launch then
    reads the input once and runs a GEMM twice as wide.  Output bytes are unchanged."""
    def pair(a, b):
        if b['dst_coff'] == a['dst_coff'] + a['cout']:
            return a, b
        if a['dst_coff'] == b['dst_coff'] + b['cout']:
            return b, a

    _merge_scan(g, _SIBLING_KEY + ('dst',), pair)


def _merge_sibling_tensors(g, loc: dict):
    """Sibling CONVs that read the same input slice with the same geometry but write into DIFFERENT
    tensors: when one writes the last channels of its tensor and the other the first channels of its
    own, the two tensors become one ([first | second], every reference remapped) and the convs one GEMM
    with N = cout_a + cout_b, as in _merge_siblings.  yolov7 (cfg/deploy/yolov7.yaml): layers 27 + 66
    (the P3 output into the next MP block's 1x1 and into the head's P3 route `[24, 1, Conv, [128, 1,
    1]]`), 40 + 54 (the same at P4) and SPPCSPC 51's cv1 + cv2 (models/common.py:271-280) — pairs of
    launches that each re-read a 52-210 MB input at bs 32.  Only the layout changes (the
    merged tensor's channel pitch); every layer's output keeps its values and its (tensor, offset) in
    layer_tensor."""
    def pair(a, b):
        if b['dst'] == a['dst'] or g.tensors[a['dst']][1] != g.tensors[b['dst']][1]:
            return None
        if a['dst_coff'] + a['cout'] == g.tensors[a['dst']][0] and b['dst_coff'] == 0:
            return a, b          # [a's tensor | b's tensor]
        if b['dst_coff'] + b['cout'] == g.tensors[b['dst']][0] and a['dst_coff'] == 0:
            return b, a          # [b's tensor | a's tensor]

    _merge_scan(g, _SIBLING_KEY, pair, loc)
