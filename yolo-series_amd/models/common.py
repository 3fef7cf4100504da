"""Layer modules of the yolov7 family — the reference's layer "plugin" names and parameter trees.

Mirror of the reference interface in models/common.py: class names (Conv, RepConv, SPPCSPC, DownC, MP, SP,
ReOrg, Concat, Shortcut, ImplicitA, ImplicitM) and attribute names (conv, bn, act, rbr_dense, rbr_1x1,
rbr_identity, rbr_reparam, cv1..cv7, m, mp, d, implicit) are identical, so reference-keyed state_dicts
 load unchanged.  The modules are parameter containers: the computation of the
whole network runs on the MI355X through the compiled plan (yv7.graph / libyv7), never layer by
layer and never on the CPU, so calling a layer directly raises.

The model's front door for real images is here too (common.py:852-1012): NMS, autoShape ("a list of images
of whatever size in, boxes in each image's own pixels out") and its result class Detections.  autoShape runs one
ragged letterbox launch, one forward, one batched NMS and one box-scaling launch per call (libyv7
yv7_letterbox_ragged / yv7_nms / yv7_scale_boxes), and Detections.render / save / show draw the boxes on the
device in one more call (yv7_draw_boxes, utils/plots.py).  URL inputs are out of scope.

Folding (Model.fuse in the reference) is restated here with the reference arithmetic:
  Conv:    fuse_conv_and_bn      utils/torch_utils.py:181-201
  RepConv: fuse_repvgg_block     models/common.py:584-643 (+ fuse_conv_bn 561-582)
"""
from __future__ import annotations

from copy import copy
from pathlib import Path

import numpy as np
import torch
import torch.nn as nn

from utils.datasets import OUT_F16_CHW, OUT_F32_CHW, autoshape_geometry, entry_channels, imread, letterbox_ragged
from utils.general import increment_path, nms_batched, non_max_suppression, scale_boxes, xyxy2xywh
from utils.plots import color_list, display_frames, plot_boxes
from utils.torch_utils import fuse_conv_and_bn, time_synchronized


def autopad(k, p=None):  # models/common.py:23-27
    if p is None:
        p = k // 2 if isinstance(k, int) else [x // 2 for x in k]
    return p


class _PlanOnly(nn.Module):
    """Layers execute only inside the compiled network (Model.forward -> libyv7)."""

    def forward(self, *args, **kwargs):
        raise RuntimeError(f'{type(self).__name__} runs only as part of models.yolo.Model.forward on a ROCm '
                           f'device (compiled plan); there is no per-layer or CPU execution path')


class MP(_PlanOnly):  # common.py:30-36
    def __init__(self, k=2):
        super().__init__()
        self.m = nn.MaxPool2d(kernel_size=k, stride=k)


class SP(_PlanOnly):  # common.py:39-45
    def __init__(self, k=3, s=1):
        super().__init__()
        self.m = nn.MaxPool2d(kernel_size=k, stride=s, padding=k // 2)


class ReOrg(_PlanOnly):  # common.py:48-53 (x(b,c,w,h) -> y(b,4c,w/2,h/2))
    pass


class Concat(_PlanOnly):  # common.py:56-62
    def __init__(self, dimension=1):
        super().__init__()
        self.d = dimension


class Shortcut(_PlanOnly):  # common.py:80-86 (x[0] + x[1])
    def __init__(self, dimension=0):
        super().__init__()
        self.d = dimension


class Conv(_PlanOnly):
    """Conv2d(bias=False) + BatchNorm2d + act (common.py:99-111); after fuse(): conv has a bias, no bn."""

    def __init__(self, c1, c2, k=1, s=1, p=None, g=1, act=True):
        super().__init__()
        self.conv = nn.Conv2d(c1, c2, k, s, autopad(k, p), groups=g, bias=False)
        self.bn = nn.BatchNorm2d(c2)
        self.act = nn.SiLU() if act is True else (act if isinstance(act, nn.Module) else nn.Identity())

    def fuse(self):
        if hasattr(self, 'bn'):
            self.conv = fuse_conv_and_bn(self.conv, self.bn)
            delattr(self, 'bn')
        return self

    def fused_weight_bias(self):
        """(W [c2,c1,k,k], b [c2]) in fp32 with BN folded, whatever the module's current state."""
        if hasattr(self, 'bn'):
            f = fuse_conv_and_bn(self.conv.float(), self.bn.float())
            return f.weight.detach().float(), f.bias.detach().float()
        b = self.conv.bias if self.conv.bias is not None else torch.zeros(self.conv.out_channels)
        return self.conv.weight.detach().float(), b.detach().float()


def _fuse_conv_bn(conv, bn):
    """RepConv.fuse_conv_bn arithmetic (common.py:561-582): returns (W*t, beta - mean*gamma/std)."""
    std = (bn.running_var + bn.eps).sqrt()
    bias = bn.bias - bn.running_mean * bn.weight / std
    t = (bn.weight / std).reshape(-1, 1, 1, 1)
    return conv.weight * t, bias


class RepConv(_PlanOnly):
    """RepVGG-style block (common.py:463-643): 3x3+BN, 1x1+BN (+ identity BN) -> one 3x3 conv when deployed."""

    def __init__(self, c1, c2, k=3, s=1, p=None, g=1, act=True, deploy=False):
        super().__init__()
        self.deploy = deploy
        self.groups = g
        self.in_channels = c1
        self.out_channels = c2
        assert k == 3
        assert autopad(k, p) == 1
        padding_11 = autopad(k, p) - k // 2
        self.act = nn.SiLU() if act is True else (act if isinstance(act, nn.Module) else nn.Identity())
        if deploy:
            self.rbr_reparam = nn.Conv2d(c1, c2, k, s, autopad(k, p), groups=g, bias=True)
        else:
            self.rbr_identity = nn.BatchNorm2d(num_features=c1) if c2 == c1 and s == 1 else None
            self.rbr_dense = nn.Sequential(nn.Conv2d(c1, c2, k, s, autopad(k, p), groups=g, bias=False),
                                           nn.BatchNorm2d(num_features=c2))
            self.rbr_1x1 = nn.Sequential(nn.Conv2d(c1, c2, 1, s, padding_11, groups=g, bias=False),
                                         nn.BatchNorm2d(num_features=c2))

    @torch.no_grad()
    def _equivalent(self):
        w3, b3 = _fuse_conv_bn(self.rbr_dense[0], self.rbr_dense[1])
        w1, b1 = _fuse_conv_bn(self.rbr_1x1[0], self.rbr_1x1[1])
        w1 = torch.nn.functional.pad(w1, [1, 1, 1, 1])
        if isinstance(self.rbr_identity, nn.BatchNorm2d):
            eye = torch.zeros(self.out_channels, self.in_channels // self.groups, 1, 1, dtype=w3.dtype)
            for i in range(self.out_channels):
                eye[i, i % (self.in_channels // self.groups), 0, 0] = 1.0
            idc = nn.Conv2d(self.in_channels, self.out_channels, 1, bias=False)
            idc.weight.data = eye
            wi, bi = _fuse_conv_bn(idc, self.rbr_identity)
            wi = torch.nn.functional.pad(wi, [1, 1, 1, 1])
        else:
            wi, bi = torch.zeros_like(w1), torch.zeros_like(b1)
        return w3 + w1 + wi, b3 + b1 + bi

    def fuse_repvgg_block(self):
        if self.deploy:
            return
        w, b = self._equivalent()
        conv = self.rbr_dense[0]
        self.rbr_reparam = nn.Conv2d(conv.in_channels, conv.out_channels, conv.kernel_size, conv.stride,
                                     conv.padding, groups=conv.groups, bias=True)
        self.rbr_reparam.weight = nn.Parameter(w.detach())
        self.rbr_reparam.bias = nn.Parameter(b.detach())
        self.deploy = True
        for name in ('rbr_identity', 'rbr_1x1', 'rbr_dense'):
            if hasattr(self, name):
                delattr(self, name)

    def fused_weight_bias(self):
        if hasattr(self, 'rbr_reparam'):
            return self.rbr_reparam.weight.detach().float(), self.rbr_reparam.bias.detach().float()
        w, b = self._equivalent()
        return w.detach().float(), b.detach().float()


class DownC(_PlanOnly):
    """Downsampling block of the e6 / d6 / e6e cfgs (common.py:181-192):
    cat(cv2(cv1(x)), cv3(mp(x))) — a 1x1 + strided 3x3 branch beside a max-pool + 1x1 branch."""

    def __init__(self, c1, c2, n=1, k=2):
        super().__init__()
        c_ = int(c1)
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c_, c2 // 2, 3, k)
        self.cv3 = Conv(c1, c2 // 2, 1, 1)
        self.mp = nn.MaxPool2d(kernel_size=k, stride=k)


class SPPCSPC(_PlanOnly):
    """CSP spatial pyramid pooling (common.py:262-280)."""

    def __init__(self, c1, c2, n=1, shortcut=False, g=1, e=0.5, k=(5, 9, 13)):
        super().__init__()
        c_ = int(2 * c2 * e)
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c1, c_, 1, 1)
        self.cv3 = Conv(c_, c_, 3, 1)
        self.cv4 = Conv(c_, c_, 1, 1)
        self.m = nn.ModuleList([nn.MaxPool2d(kernel_size=x, stride=1, padding=x // 2) for x in k])
        self.cv5 = Conv(4 * c_, c_, 1, 1)
        self.cv6 = Conv(c_, c_, 3, 1)
        self.cv7 = Conv(2 * c_, c2, 1, 1)


class ImplicitA(_PlanOnly):  # common.py:433-443
    def __init__(self, channel, mean=0., std=.02):
        super().__init__()
        self.channel = channel
        self.mean = mean
        self.std = std
        self.implicit = nn.Parameter(torch.zeros(1, channel, 1, 1))
        nn.init.normal_(self.implicit, mean=self.mean, std=self.std)


class ImplicitM(_PlanOnly):  # common.py:446-456
    def __init__(self, channel, mean=1., std=.02):
        super().__init__()
        self.channel = channel
        self.mean = mean
        self.std = std
        self.implicit = nn.Parameter(torch.ones(1, channel, 1, 1))
        nn.init.normal_(self.implicit, mean=self.mean, std=self.std)


class NMS(nn.Module):  # common.py:852-862
    conf = 0.25     # confidence threshold
    iou = 0.45      # IoU threshold
    classes = None  # (optional list) filter by class

    def forward(self, x):
        return non_max_suppression(x[0], conf_thres=self.conf, iou_thres=self.iou, classes=self.classes)


def _as_hwc3(im):
    """common.py:906-908 on one decoded image: CHW -> HWC when shape[0] < 5, alpha dropped, grey tiled to 3."""
    is_u8 = (isinstance(im, np.ndarray) and im.dtype == np.uint8) or \
            (isinstance(im, torch.Tensor) and im.dtype == torch.uint8)
    if not is_u8:
        raise ValueError(f'autoShape: images must be uint8 (got {getattr(im, "dtype", type(im).__name__)}); '
                         f'scale and convert before the call')
    if isinstance(im, torch.Tensor):
        if not im.is_cuda or im.ndim != 3 or im.shape[2] != 3:
            raise ValueError(f'autoShape: a tensor image must be uint8 [H, W, 3] on the HIP device, got '
                             f'{tuple(im.shape)} on {im.device}')
        return im
    if im.ndim not in (2, 3):
        raise ValueError(f'autoShape: expected an HWC, CHW or HW image, got shape {im.shape}')
    if im.shape[0] < 5:
        im = im.transpose((1, 2, 0))
    return im[:, :, :3] if im.ndim == 3 else np.tile(im[:, :, None], 3)


def _as_hwc(im, C):
    """One decoded image as the uint8 [H, W, C] frame of a C-channel model (autoShape with a frame mode): [H, W]
    becomes [H, W, 1] for C = 1, [C, H, W] is transposed when only its first axis can be the channels; nothing is
    dropped or tiled, so any other channel count is an error."""
    is_t = isinstance(im, torch.Tensor)
    if not ((isinstance(im, np.ndarray) and im.dtype == np.uint8) or (is_t and im.dtype == torch.uint8)):
        raise ValueError(f'autoShape: images must be uint8 (got {getattr(im, "dtype", type(im).__name__)}); '
                         f'scale and convert before the call')
    if is_t and not im.is_cuda:
        raise ValueError(f'autoShape: a tensor image must be on the HIP device, got {im.device}')
    shape = tuple(im.shape)
    if im.ndim == 2 and C == 1:
        im = im[:, :, None]
    if im.ndim == 3 and im.shape[0] == C != im.shape[2]:
        im = im.permute(1, 2, 0) if is_t else im.transpose((1, 2, 0))
    if im.ndim != 3 or im.shape[2] != C:
        raise ValueError(f'autoShape: expected an image of {C} channels (HWC or CHW), got shape {shape}')
    return im


class autoShape(nn.Module):  # common.py:865-932
    """Input-robust model wrapper: filenames, PIL images, uint8 numpy arrays (HWC / CHW / HW) or uint8 HWC HIP
    tensors, one or a list, any sizes, RGB -> Detections.  A float tensor goes straight to the model.
    frames (utils.datasets.FRAME_MODES) states how files and images become the frames of a model of another
    channel count: files through imread(path, frames), PIL images converted to that mode (taken as they are for
    'raw'), arrays and HIP tensors as [H, W, C] / [C, H, W] of exactly the model's channels, in their own order.
    With frames=None a model of another count is refused, as ever."""
    conf = 0.25     # NMS confidence threshold
    iou = 0.45      # NMS IoU threshold
    classes = None  # (optional list) filter by class

    def __init__(self, model, frames=None):
        super().__init__()
        self.ch = entry_channels(model, frames)
        self.frames = frames
        self.model = model.eval()

    def autoshape(self):
        print('autoShape already enabled, skipping... ')
        return self

    @torch.no_grad()
    def forward(self, imgs, size=640, augment=False, profile=False):
        t = [time_synchronized()]
        p = next(self.model.parameters())   # for device and type
        if isinstance(imgs, torch.Tensor):
            return self.model(imgs.to(p.device).type_as(p), augment, profile)
        if p.device.type != 'cuda':
            raise RuntimeError('autoShape runs on a ROCm (MI355X) device via libyv7; move the model to cuda')

        n, imgs = (len(imgs), list(imgs)) if isinstance(imgs, (list, tuple)) else (1, [imgs])
        files = []
        for i, im in enumerate(imgs):
            f = f'image{i}'
            if self.frames is not None:
                if isinstance(im, (str, Path)):
                    im, f = imread(im, self.frames), str(im)
                elif hasattr(im, 'convert') and hasattr(im, 'size'):   # PIL Image
                    f = getattr(im, 'filename', f) or f
                    im = np.asarray(im if self.frames == 'raw' else im.convert(self.frames))
                files.append(Path(f).with_suffix('.jpg').name)
                imgs[i] = _as_hwc(im, self.ch)
                continue
            if isinstance(im, (str, Path)):
                from PIL import Image
                if str(im).startswith('http'):
                    raise ValueError('autoShape: URLs are not supported (this package has no network code)')
                with Image.open(im) as pil:
                    im, f = np.asarray(pil.convert('RGB')), str(im)
            elif hasattr(im, 'convert') and hasattr(im, 'size'):   # PIL Image
                im, f = np.asarray(im), getattr(im, 'filename', f) or f
            files.append(Path(f).with_suffix('.jpg').name)
            imgs[i] = _as_hwc3(im)
        shape0 = [tuple(im.shape[:2]) for im in imgs]
        shape1, geoms, descs = autoshape_geometry(shape0, size, int(self.stride.max()))
        x = letterbox_ragged(imgs, geoms, shape1, swap_rb=False, device=p.device,
                             out_kind=OUT_F16_CHW if p.dtype == torch.float16 else OUT_F32_CHW)
        t.append(time_synchronized())

        y = self.model(x, augment, profile)[0]
        t.append(time_synchronized())

        det, _, cnt = nms_batched(y, conf_thres=self.conf, iou_thres=self.iou, classes=self.classes)
        views = scale_boxes(det, cnt, descs, round_boxes=False, views=True)
        counts = cnt.tolist()   # the one host sync: variable-length outputs
        pred, xywh, xyxyn, xywhn = ([v[i, :c] for i, c in enumerate(counts)] for v in (det, *views))
        t.append(time_synchronized())
        return Detections(imgs, pred, files, t, self.names, x.shape, views=(xywh, xyxyn, xywhn), batch=(det, cnt))


class Detections:  # common.py:935-1012
    """Results of one autoShape call: per image pred = xyxy [n, 6] (x1, y1, x2, y2, conf, cls) in the image's own
    pixels, and the views xywh (centre, size), xyxyn, xywhn (normalised by the image's w, h)."""

    def __init__(self, imgs, pred, files, times=None, names=None, shape=None, views=None, batch=None):
        self.imgs = imgs      # list of images as given (numpy arrays or HIP tensors, HWC)
        self._batch = batch   # autoShape's (det [B, max_det, 6], count [B]) that pred's rows are views of
        self.pred = pred      # list of tensors pred[0] = (xyxy, conf, cls)
        self.names = names    # class names
        self.files = files    # image filenames
        self.xyxy = pred
        if views is None:     # common.py:940-948 in tensor math, for results assembled by hand
            gn = [torch.tensor([*[im.shape[i] for i in (1, 0, 1, 0)], 1., 1.], device=x.device)
                  for im, x in zip(imgs, pred)]
            xywh = [xyxy2xywh(x) for x in pred]
            views = xywh, [x / g for x, g in zip(pred, gn)], [x / g for x, g in zip(xywh, gn)]
        self.xywh, self.xyxyn, self.xywhn = views
        self.n = len(self.pred)   # number of images (batch size)
        self.t = tuple((times[i + 1] - times[i]) * 1000 / self.n for i in range(3)) if times else (0., 0., 0.)
        self.s = shape            # inference BCHW shape

    def _summary(self, i):
        """display()'s line for image i: 'image 1/2: 1080x810 4 persons, 1 bus'."""
        img, pred = self.imgs[i], self.pred[i]
        line = f'image {i + 1}/{self.n}: {img.shape[0]}x{img.shape[1]} '
        for c in pred[:, -1].unique():
            k = int((pred[:, -1] == c).sum())   # detections per class
            line += f"{k} {self.names[int(c)]}{'s' * (k > 1)}, "
        return line.rstrip(', ')

    def print(self):
        for i in range(self.n):
            print(self._summary(i))
        print(f'Speed: %.1fms pre-process, %.1fms inference, %.1fms NMS per image at shape {tuple(self.s)}' % self.t)

    def _draw(self, what):
        """The boxes of every image drawn by one plot_boxes call (Detections.display's plot_one_box loop,
        common.py:965-968: forward order, 'name conf' labels, color_list(), the per-image line thickness)."""
        if any(not (isinstance(p, torch.Tensor) and p.is_cuda) for p in self.pred):
            raise NotImplementedError(f'Detections.{what}: drawing runs on the ROCm device (libyv7 yv7_draw_boxes); '
                                      f'these predictions are CPU tensors and there is no CPU drawing path')
        if self.n == 0:
            return
        if self._batch is not None:
            det, cnt = self._batch
        else:   # results assembled by hand: the fixed-shape form the kernel reads
            dev = self.pred[0].device
            cnt = torch.tensor([len(p) for p in self.pred], dtype=torch.int32, device=dev)
            det = torch.zeros((self.n, max(int(cnt.max()), 1), 6), dtype=torch.float32, device=dev)
            for i, p in enumerate(self.pred):
                det[i, :len(p)] = p
        frames = self.imgs
        if any(im.shape[2] != 3 for im in frames):   # the drawing is 3-channel: draw on display copies
            frames = display_frames(frames, det.device)
        out = plot_boxes(frames, det, cnt, names=self.names, colors=color_list(), reverse=False)
        host = [i for i, im in enumerate(self.imgs) if isinstance(im, np.ndarray)]
        for i, im in enumerate(self.imgs):
            if isinstance(im, torch.Tensor):
                self.imgs[i] = out[i]
        if host:   # one download for the batch
            flat = torch.cat([out[i].reshape(-1) for i in host]).cpu().numpy()
            off = 0
            for i in host:
                self.imgs[i] = flat[off:off + out[i].numel()].reshape(tuple(out[i].shape))
                off += out[i].numel()

    def show(self):
        from PIL import Image
        for im, f in zip(self.render(), self.files):
            Image.fromarray(im.cpu().numpy() if isinstance(im, torch.Tensor) else im).show(f)

    def save(self, save_dir='runs/hub/exp'):
        from PIL import Image
        imgs = self.render()   # raises for CPU predictions before anything is written
        save_dir = increment_path(save_dir, exist_ok=save_dir != 'runs/hub/exp')   # common.py:984-987
        Path(save_dir).mkdir(parents=True, exist_ok=True)
        for i, (im, f) in enumerate(zip(imgs, self.files)):
            Image.fromarray(im.cpu().numpy() if isinstance(im, torch.Tensor) else im).save(Path(save_dir) / f)
            print(f"{'Saved' * (i == 0)} {f}", end=',' if i < self.n - 1 else f' to {save_dir}\n')

    def render(self):
        self._draw('render')
        return self.imgs

    def pandas(self):
        """A copy whose four views are pandas DataFrames, i.e. print(results.pandas().xyxy[0])."""
        import pandas as pd
        new = copy(self)
        ca = 'xmin', 'ymin', 'xmax', 'ymax', 'confidence', 'class', 'name'
        cb = 'xcenter', 'ycenter', 'width', 'height', 'confidence', 'class', 'name'
        for k, cols in zip(('xyxy', 'xyxyn', 'xywh', 'xywhn'), (ca, ca, cb, cb)):
            rows = [[r[:5] + [int(r[5]), self.names[int(r[5])]] for r in x.tolist()] for x in getattr(self, k)]
            setattr(new, k, [pd.DataFrame(r, columns=cols) for r in rows])
        return new

    def tolist(self):
        """One Detections per image, its list fields unwrapped, i.e. 'for result in results.tolist():'."""
        out = []
        for i in range(self.n):
            d = Detections([self.imgs[i]], [self.pred[i]], [self.files[i]], None, self.names, self.s,
                           views=([self.xywh[i]], [self.xyxyn[i]], [self.xywhn[i]]))
            d.t = self.t
            for k in ('imgs', 'pred', 'xyxy', 'xyxyn', 'xywh', 'xywhn'):
                setattr(d, k, getattr(d, k)[0])   # pop out of list
            out.append(d)
        return out

    def __len__(self):
        return self.n
