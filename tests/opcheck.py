"""Per-op parity of a libyv7 plan: every op's output against a plain PyTorch fp32 reference of the
same op, computed from the op's own input as the plan left it in the workspace.

This isolates each kernel from the error the network accumulates upstream, so it checks exactly the
dispatch a forward took (tile-count dependent kernel choice, split-K, persistent rings, the pooled
1x1, the fused stem, the head).  The references are the reference module's arithmetic:
  CONV      act(conv2d(x, W, b, s, k//2))       models/common.py:110-111 (Conv.fuseforward), 498-500 (RepConv)
            with pool = 2: the MP in front       common.py:30-36
  STEM      the two Convs of layers 0-1          common.py:110-111, with the kernel's own fp16 steps
                                                 (conv A stored in fp16, SiLU's -log2(e) folded into it)
  MAXPOOL   F.max_pool2d(x, k, s, pad)           common.py:30-45, 271 (SPPCSPC cascade 5∘5 = 9, 5∘5∘5 = 13)
  UPSAMPLE  nearest x2                           cfg nn.Upsample(None, 2, 'nearest')
  COPY      the concat slice                     common.py:56-62
  DETECT    1x1 conv + bias (raw logits) and the decode   models/yolo.py:46-57
Convolutions run as sums of per-tap fp32 matmuls on the device (no MIOpen: nothing is compiled at
run time).  Tolerances: an fp16 output within one fp16 ulp of the fp32 reference (+1e-4 of the op's
rms for the accumulation order; two ulps for the fused stem, whose intermediate is fp16); fp32 outputs within 1e-5 |ref| + 1e-4 rms; max / upsample / copy exact.
An output that is not finite is an element off; a reference that is not finite is an error naming the op's input.
check_ops reads the image interiors only (it pads its references itself), so it does not see a kernel that writes the
zero frame around an image: tests/test_gemm_edges.py and tests/test_family_gpu.py check the frames (helpers.bordered).

check_ops checks DETECT through the raw logits, and a forward that returns them never runs the persistent heads
(csrc/conv_det.hip).  check_detect_z checks z alone: per level a float64 conv + decode of the op's own input
against z's rows, within the bound check_z_level derives from the two tolerances above (raw logits 1e-4 of
their scale, decode 1e-5).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from yv7 import _lib as L


def _act(y, act):
    if act == L.ACT_SILU:
        return F.silu(y)
    if act == L.ACT_LEAKY:
        return F.leaky_relu(y, 0.1)
    return y


def _weights(plan, blob, o, cin=None):
    """Packed weights of a CONV / DETECT op as fp32 [cout, k, k, cin] (plan dtype values) + bias."""
    k, cout = o.get('k', 1), o['cout']
    cin = o['cin'] if cin is None else cin
    es = 2 if plan.dtype == L.DT_F16 else 4
    kpad = (k * k * cin + 63) // 64 * 64
    cpad = (cout + 31) // 32 * 32
    w = blob[o['w_off']:o['w_off'] + cpad * kpad * es].view(torch.float16 if es == 2 else torch.float32)
    w = w.view(cpad, kpad)[:cout, :k * k * cin].float().reshape(cout, k, k, cin)
    b = blob[o['b_off']:o['b_off'] + cout * 4].view(torch.float32).clone()
    return w, b


def conv_ref(x, w, b, s, act):
    """act(conv2d) of an NHWC fp32 batch x [B,H,W,cin] with w [cout,k,k,cin], pad k//2, as per-tap
    fp32 matmuls -> NHWC fp32."""
    k = w.shape[1]
    pad = k // 2
    B, H, W, C = x.shape
    Ho, Wo = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    xp = F.pad(x, [0, 0, pad, pad, pad, pad]) if pad else x
    y = b.to(x.device).expand(B * Ho * Wo, -1).clone()
    for r in range(k):
        for c in range(k):
            xs = xp[:, r:r + (Ho - 1) * s + 1:s, c:c + (Wo - 1) * s + 1:s, :].reshape(-1, C)
            y += xs @ w[:, r, c, :].t().to(x.device)
    return _act(y, act).view(B, Ho, Wo, -1)


def _ulp_check(got, ref, what, fp16, ulps=1, xin=None):
    """A non-finite `got` where `ref` is finite counts as an element off (|got - ref| > tol is false for a
    NaN); a non-finite `ref` is an error of its own that names the op's input `xin` (where given): the
    reference was built from what the plan left there."""
    got, ref = got.float(), ref.float()
    ref_ok = torch.isfinite(ref)
    if not ref_ok.all():
        src = '' if xin is None else (f'; its input: max |x| {xin.float().abs().max().item():.4g}, '
                                      f'finite {bool(torch.isfinite(xin).all())}')
        raise AssertionError(f'{what}: {int((~ref_ok).sum())} of {ref.numel()} reference values not finite' + src)
    rms = ref.pow(2).mean().sqrt().item()
    if fp16:   # `ulps` fp16 ulps of the larger of the two (a value just under a power of two may round up)
        tol = torch.maximum(ref.abs(), got.abs()) * 2.0 ** -11 * (2 * ulps) + 1e-4 * rms + 1e-7
    else:
        tol = ref.abs() * 1e-5 + 1e-4 * rms + 1e-12
    got_ok = torch.isfinite(got)
    d = torch.where(got_ok, (got - ref).abs(), torch.full_like(ref, float('inf')))
    bad = ~got_ok | (d > tol)
    nbad = int(bad.sum())
    worst = (d / (ref.abs() + rms + 1e-30)).max().item()
    assert nbad == 0, (f'{what}: {nbad} of {d.numel()} elements off ({int((~got_ok).sum())} not finite, '
                       f'max |d| {d.max().item():.3g}, rms(ref) {rms:.3g}, worst rel {worst:.3g})')
    return worst


def check_ops(plan, x, B, H, W, raw=None, z=None, skip_fp8=True):
    """Check every op of the last forward of `plan` on input x [B,3,H,W].  Returns {op: worst rel err}."""
    g = plan.graph
    blob = g.weight_blob().to(plan.device)
    fp16 = plan.dtype == L.DT_F16
    es_dt = torch.float16 if fp16 else torch.float32
    tv = lambda t: plan.tensor_view(t, B, H, W)   # interior NHWC views  # noqa: E731
    out = {}
    det_levels = []
    for i, o in enumerate(g.ops):
        kind = o['kind']
        what = f'op {i} ({kind}: {o.get("cin", 0)}->{o["cout"]} k{o.get("k", 1)} s{o.get("s", 1)})'
        if kind == L.OP_INPUT:
            t = tv(o['dst'])
            if o.get('k', 1) == 2:   # ReOrg (common.py:52-53) fused into the packing
                xr = torch.cat([x[..., ::2, ::2], x[..., 1::2, ::2], x[..., ::2, 1::2], x[..., 1::2, 1::2]], 1)
            else:
                xr = x
            ref = xr.to(es_dt).permute(0, 2, 3, 1)
            got = t[..., :ref.shape[-1]]
            assert torch.equal(got, ref), what
            out[i] = 0.0
        elif kind == L.OP_CONV:
            if o.get('wfmt', 0) == L.WFMT_FP8:
                if skip_fp8:
                    continue
                raise NotImplementedError('fp8 ops: tests/test_fp8.py')
            xin = tv(o['src'])[..., o['src_coff']:o['src_coff'] + o['cin']].float()
            s = o['s']
            if o.get('pool', 0) == 2:
                xin = F.max_pool2d(xin.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
                s = 1
            w, b = _weights(plan, blob, o)
            ref = conv_ref(xin, w, b, s, o['act'])
            got = tv(o['dst'])[..., o['dst_coff']:o['dst_coff'] + o['cout']]
            out[i] = _ulp_check(got, ref, what, fp16, xin=xin)
        elif kind == L.OP_STEM:
            # csrc/stem.hip's arithmetic: with SiLU on both convs, conv A's weights / bias are
            # pre-scaled by -log2(e) (weights rounded to fp16 again), A is stored in fp16 as
            # -log2(e) * silu(a), conv B's bias is scaled the same way and its epilogue undoes it
            reorg = o['cin'] == 12   # the w6 front end: ReOrg (common.py:52-53) + conv A on 12 channels
            xr = torch.cat([x[..., ::2, ::2], x[..., 1::2, ::2], x[..., ::2, 1::2], x[..., 1::2, 1::2]], 1) if reorg else x
            xin = xr.to(es_dt).float().permute(0, 2, 3, 1).contiguous()
            wa, ba = _weights(plan, blob, dict(o, cin=16 if reorg else 3))
            wa = wa[..., :o['cin']]
            ob = dict(o, cin=o['cout'], cout=o['cout2'], w_off=o['w2_off'], b_off=o['b2_off'])
            wb, bb = _weights(plan, blob, ob)
            if o['act'] == L.ACT_SILU and o['act2'] == L.ACT_SILU:
                nl2e = -1.4426950408889634
                za = conv_ref(xin, (wa * nl2e).half().float(), ba * nl2e, o['s'], L.ACT_NONE)
                a = (za / (1.0 + torch.exp2(za))).half().float()
                zb = conv_ref(a, wb, bb * nl2e, 2, L.ACT_NONE)
                ref = (zb * -0.6931471805599453) / (1.0 + torch.exp2(zb))
            else:
                a = conv_ref(xin, wa, ba, o['s'], o['act']).to(es_dt).float()
                ref = conv_ref(a, wb, bb, 2, o['act2'])
            got = tv(o['dst'])[..., o['dst_coff']:o['dst_coff'] + o['cout2']]
            # conv A's fp16 rounding flips by an ulp where its fp32 sum (approximate exp2 / rcp in the
            # SiLU) lands on the other side of a rounding step than the reference's; conv B carries
            # such a flip (up to ulp(|A|) x |w|, ~1e-3 for the large A values) into its output.  So:
            # two ulps everywhere but a few 1e-4 of the elements, which stay within 5e-3 of the rms
            got, ref = got.float(), ref.float()
            rms = ref.pow(2).mean().sqrt().item()
            d = (got - ref).abs()
            loose = int((d > torch.maximum(ref.abs(), got.abs()) * 2.0 ** -9 + 1e-4 * rms).sum())
            assert loose <= 1e-3 * d.numel(), f'{what}: {loose} of {d.numel()} elements beyond two ulps'
            assert d.max().item() <= 5e-3 * rms, f'{what}: max |d| {d.max().item():.3g} (rms {rms:.3g})'
            out[i] = (d / (ref.abs() + rms)).max().item()
        elif kind == L.OP_MAXPOOL:
            xin = tv(o['src'])[..., o['src_coff']:o['src_coff'] + o['cout']]
            ref = F.max_pool2d(xin.permute(0, 3, 1, 2).float(), o['k'], o['s'], o['pad']).permute(0, 2, 3, 1)
            got = tv(o['dst'])[..., o['dst_coff']:o['dst_coff'] + o['cout']]
            assert torch.equal(got.float(), ref), what
            out[i] = 0.0
        elif kind == L.OP_UPSAMPLE:
            xin = tv(o['src'])[..., o['src_coff']:o['src_coff'] + o['cout']]
            ref = xin.repeat_interleave(2, 1).repeat_interleave(2, 2)
            got = tv(o['dst'])[..., o['dst_coff']:o['dst_coff'] + o['cout']]
            assert torch.equal(got, ref), what
            out[i] = 0.0
        elif kind == L.OP_COPY:
            xin = tv(o['src'])[..., o['src_coff']:o['src_coff'] + o['cout']]
            got = tv(o['dst'])[..., o['dst_coff']:o['dst_coff'] + o['cout']]
            assert torch.equal(got, xin), what
            out[i] = 0.0
        elif kind == L.OP_DETECT:
            det_levels.append((i, o))
    if raw is not None:
        # raw logits [B, na, ny, nx, no] per level: 1x1 conv + bias in fp32 (yolo.py:46-50)
        for (i, o), xs in zip(sorted(det_levels, key=lambda t: t[1]['level']), raw):
            xin = tv(o['src'])[..., o['src_coff']:o['src_coff'] + o['cin']].float()
            w, b = _weights(plan, blob, o)
            ref = conv_ref(xin, w, b, 1, L.ACT_NONE)     # [B, ny, nx, na*no]
            Bq, ny, nx, _ = ref.shape
            ref = ref.view(Bq, ny, nx, plan.na, plan.no).permute(0, 3, 1, 2, 4)
            scale = max(1.0, ref.abs().max().item())
            d = (xs.float() - ref).abs().max().item()
            assert d <= 1e-4 * scale, f'op {i} DETECT level {o["level"]}: raw logits max |d| {d:.3g} (scale {scale:.3g})'
            out[i] = d / scale
        if z is not None:
            # decode of the GPU's own logits, the reference's op order (yolo.py:52-57)
            zs, row = [], 0
            for (i, o), xs in zip(sorted(det_levels, key=lambda t: t[1]['level']), raw):
                lvl = o['level']
                Bq, na, ny, nx, no = xs.shape
                y = xs.float().sigmoid()
                yv, xv = torch.meshgrid(torch.arange(ny, device=y.device), torch.arange(nx, device=y.device),
                                        indexing='ij')
                grid = torch.stack((xv, yv), 2).view(1, 1, ny, nx, 2).float()
                ag = torch.tensor(g.anchor_grid, device=y.device).view(g.nl, 1, g.na, 1, 1, 2)[lvl]
                y[..., 0:2] = (y[..., 0:2] * 2. - 0.5 + grid) * g.stride[lvl]
                y[..., 2:4] = (y[..., 2:4] * 2) ** 2 * ag
                zs.append(y.view(Bq, -1, no))
            zr = torch.cat(zs, 1)
            sc = zr.abs().clamp(min=1.0)
            d = ((z.float() - zr).abs() / sc).max().item()
            assert d <= 1e-5, f'Detect decode: max rel |d| {d:.3g}'
    return out


def decode_ref(logits, stride, anchors):
    """The Detect decode (yolo.py:52-57) of one level in the logits' own precision: logits [B, ny, nx, na*no]
    (a 1x1 conv's NHWC output), anchors [na, 2] in pixels -> that level's z rows [B, na*ny*nx, no] in z's row
    order (anchor, y, x)."""
    B, ny, nx, c = logits.shape
    na = anchors.shape[0]
    no = c // na
    y = logits.view(B, ny, nx, na, no).permute(0, 3, 1, 2, 4).sigmoid()
    yv, xv = torch.meshgrid(torch.arange(ny, device=y.device), torch.arange(nx, device=y.device), indexing='ij')
    grid = torch.stack((xv, yv), 2).view(1, 1, ny, nx, 2).to(y.dtype)
    ag = anchors.to(y).view(1, na, 1, 1, 2)
    y = torch.cat(((y[..., 0:2] * 2. - 0.5 + grid) * stride, (y[..., 2:4] * 2) ** 2 * ag, y[..., 4:]), -1)
    return y.reshape(B, na * ny * nx, no)


def check_z_level(zl, logits, stride, anchors, what):
    """One level's z rows zl [B, na*ny*nx, no] against the float64 decode of float64 reference logits
    [B, ny, nx, na*no] (anchors [na, 2] in pixels).  Returns the worst |z - z_ref| / bound.

    The bound is the two errors the project already allows, added: the decode's 1e-5 max(|z_ref|, 1), and
    the logits' dl = 1e-4 max(1, max |logit_ref|) carried through the decode by its largest slope —
      x, y      (2 s - 0.5 + g) stride   d/dl = 2 s (1 - s) stride        <= 0.5 stride
      w, h      (2 s)^2 anchor           d/dl = 8 s^2 (1 - s) anchor      <= 32/27 anchor (at s = 2/3)
      obj, cls  s                        d/dl = s (1 - s)                 <= 0.25
    (s = sigmoid(logit); the slopes are global maxima, so the bound holds for any perturbation of at most
    dl, not only to first order).  A z element that is not finite fails."""
    logits = logits.double()
    zr = decode_ref(logits, float(stride), anchors.double())
    assert zl.shape == zr.shape, f'{what}: z rows {tuple(zl.shape)}, reference {tuple(zr.shape)}'
    na, no = anchors.shape[0], zr.shape[-1]
    dl = 1e-4 * max(1.0, logits.abs().max().item())
    slope = torch.full((na, 1, no), 0.25 * dl, dtype=torch.float64, device=zr.device)
    slope[..., 0:2] = 0.5 * float(stride) * dl
    slope[..., 2:4] = (32.0 / 27.0) * dl * anchors.double().to(zr.device).view(na, 1, 2)
    bound = 1e-5 * zr.abs().clamp(min=1.0) + slope.expand(na, zr.shape[1] // na, no).reshape(1, -1, no)
    finite = torch.isfinite(zl)
    assert finite.all(), f'{what}: {int((~finite).sum())} of {zl.numel()} z elements not finite'
    ratio = (zl.double() - zr).abs() / bound
    worst = ratio.max().item()
    if worst > 1.0:
        b, r, c = (int(v) for v in (ratio == ratio.max()).nonzero()[0])
        raise AssertionError(f'{what}: {int((ratio > 1).sum())} of {ratio.numel()} z elements beyond the bound, worst '
                             f'{worst:.3g} x at image {b} level row {r} column {c}: {zl[b, r, c].item():.6g} vs '
                             f'{zr[b, r, c].item():.6g}')
    return worst


def check_detect_z(plan, B, H, W, z):
    """z [B, N, no] of the last forward against a float64 reference that needs no raw logits: per DETECT op,
    the 1x1 conv of the op's own input slice (as the plan left it in the workspace) with its packed weights and
    bias in float64, decoded in float64 (check_z_level).  Returns {level: (op index, worst ratio to the bound)}."""
    g = plan.graph
    blob = g.weight_blob().to(plan.device)
    assert tuple(z.shape) == (B, plan.num_rows(H, W), plan.no), tuple(z.shape)
    out, row = {}, 0
    for i, o in sorted(((i, o) for i, o in enumerate(g.ops) if o['kind'] == L.OP_DETECT), key=lambda t: t[1]['level']):
        lvl = o['level']
        xin = plan.tensor_view(o['src'], B, H, W)[..., o['src_coff']:o['src_coff'] + o['cin']]
        what = f'op {i} DETECT level {lvl} ({o["cin"]}->{o["cout"]} @{xin.shape[1]}x{xin.shape[2]})'
        assert torch.isfinite(xin).all(), f'{what}: its input is not finite'
        w, b = _weights(plan, blob, o)
        logits = conv_ref(xin.double(), w.double(), b.double(), 1, L.ACT_NONE)
        anchors = torch.tensor(g.anchor_grid, dtype=torch.float64, device=z.device).view(g.nl, g.na, 2)[lvl]
        n = g.na * xin.shape[1] * xin.shape[2]
        out[lvl] = (i, check_z_level(z[:, row:row + n], logits, g.stride[lvl], anchors, what))
        row += n
    assert row == z.shape[1], (row, z.shape)
    return out


def kernel_summary(out):
    worst = max(out.items(), key=lambda kv: kv[1]) if out else (None, 0.0)
    return f'{len(out)} ops checked, worst rel err {worst[1]:.3g} at op {worst[0]}'


def rms_rel(got, ref):
    rms = ref.float().pow(2).mean().sqrt().item()
    return (got.float() - ref.float()).pow(2).mean().sqrt().item() / max(rms, 1e-3)
