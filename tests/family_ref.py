"""CPU reference of the whole yolov7 family, DownC and Shortcut included: a plain torch restatement of
forward_once (reference models/yolo.py:601-631) over a fused models.yolo.Model's own modules, in the
reference's op order, in fp32 or float64.

The oracle (oracle/yolo_ref.py) parses cfg dicts of the first three models and knows neither DownC nor
Shortcut; it is the yardstick of every earlier test and stays as it is.  This helper reads the weights
from the product Model after fuse() instead of folding a state_dict itself, so it depends on
Model.fuse — which tests/test_checkpoint.py pins against the oracle's folds — and on nothing in yv7.
tests/test_family_cpu.py checks it against oracle.yolo_ref.forward to the last bit in float64.

Per layer:
  Conv / RepConv   act(F.conv2d(x, W, b, s, pad))          common.py:110-111, 498-500
  DownC            cat(cv2(cv1(x)), cv3(mp(x)))            common.py:191-192
  Shortcut         x[0] + x[1]                             common.py:85-86
  SPPCSPC          common.py:276-280
  MP / SP          common.py:30-45;  ReOrg common.py:52-53;  Concat common.py:61-62;  nn.Upsample
  Detect           1x1 conv, then the decode of yolo.py:42-63 (oracle.yolo_ref.detect_decode's arithmetic)
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from models.common import MP, SP, SPPCSPC, Concat, Conv, DownC, ReOrg, RepConv, Shortcut
from models.yolo import Detect


def _act(m, x):
    a = m.act
    if isinstance(a, nn.SiLU):
        return F.silu(x)
    if isinstance(a, nn.LeakyReLU):
        return F.leaky_relu(x, a.negative_slope)
    assert isinstance(a, nn.Identity), type(a)
    return x


def _conv(m, x):
    """A fused Conv / RepConv: act(conv2d) with the module's own folded weights, in x's dtype."""
    c = m.conv if isinstance(m, Conv) else m.rbr_reparam
    assert c.bias is not None, 'family_ref runs on a fused model (Model.fuse())'
    return _act(m, F.conv2d(x, c.weight.detach().to(x.dtype), c.bias.detach().to(x.dtype), c.stride, c.padding))


def _decode(det, raw):
    """Detect.forward's inference branch (yolo.py:46-63) on the per-level conv outputs."""
    z, xs = [], []
    for i, v in enumerate(raw):
        bs, _, ny, nx = v.shape
        v = v.view(bs, det.na, det.no, ny, nx).permute(0, 1, 3, 4, 2).contiguous()
        xs.append(v)
        yv, xv = torch.meshgrid([torch.arange(ny), torch.arange(nx)], indexing='ij')
        grid = torch.stack((xv, yv), 2).view((1, 1, ny, nx, 2)).to(v.dtype)
        ag = det.anchor_grid[i].detach().to(v.dtype).view(1, det.na, 1, 1, 2)
        y = v.sigmoid()
        y[..., 0:2] = (y[..., 0:2] * 2. - 0.5 + grid) * det.stride[i].to(v.dtype)
        y[..., 2:4] = (y[..., 2:4] * 2) ** 2 * ag
        z.append(y.view(bs, -1, det.no))
    return torch.cat(z, 1), xs


@torch.no_grad()
def forward(model, x, dtype=torch.float32, return_all=False):
    """(z, xs) of the fused `model` on x [B,3,H,W], computed in `dtype`; return_all: also {layer: output}."""
    x = x.to(dtype)
    y, outs = [], {}
    for m in model.model:
        if m.f != -1:
            x = y[m.f] if isinstance(m.f, int) else [x if j == -1 else y[j] for j in m.f]
        if isinstance(m, (Conv, RepConv)):
            x = _conv(m, x)
        elif isinstance(m, DownC):
            x = torch.cat((_conv(m.cv2, _conv(m.cv1, x)), _conv(m.cv3, m.mp(x))), dim=1)
        elif isinstance(m, Shortcut):
            x = x[0] + x[1]
        elif isinstance(m, SPPCSPC):
            x1 = _conv(m.cv4, _conv(m.cv3, _conv(m.cv1, x)))
            y1 = _conv(m.cv6, _conv(m.cv5, torch.cat([x1] + [p(x1) for p in m.m], 1)))
            y2 = _conv(m.cv2, x)
            x = _conv(m.cv7, torch.cat((y1, y2), dim=1))
        elif isinstance(m, (MP, SP)):
            x = m.m(x)
        elif isinstance(m, Concat):
            x = torch.cat(x, m.d)
        elif isinstance(m, nn.Upsample):
            x = F.interpolate(x, scale_factor=float(m.scale_factor), mode=m.mode)
        elif isinstance(m, ReOrg):
            x = torch.cat([x[..., ::2, ::2], x[..., 1::2, ::2], x[..., ::2, 1::2], x[..., 1::2, 1::2]], 1)
        elif isinstance(m, Detect):
            assert not hasattr(m, 'ia'), 'family_ref runs on a fused model (Model.fuse())'
            raw = [F.conv2d(x[j], m.m[j].weight.detach().to(dtype), m.m[j].bias.detach().to(dtype))
                   for j in range(m.nl)]
            x = _decode(m, raw)
        else:
            raise NotImplementedError(type(m).__name__)
        if return_all:
            outs[m.i] = x
        y.append(x if m.i in model.save else None)
    return (x, outs) if return_all else x
