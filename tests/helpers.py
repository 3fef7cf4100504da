"""Shared fixtures: product model + seeded synthetic weights, and the oracle fed the same weights."""
from __future__ import annotations

import ctypes
import functools

import torch

from models.yolo import Model
from yv7 import _lib as L
from yv7.synthetic import synthetic_frames, synthetic_state_dict


@functools.lru_cache(maxsize=None)
def model_and_weights(name: str, seed: int = 0):
    """(unfused product Model with synthetic weights, state_dict) — cached per (name, seed)."""
    torch.manual_seed(seed)
    m = Model(name)
    sd = synthetic_state_dict(m, seed=seed)
    return m, sd


@functools.lru_cache(maxsize=None)
def oracle_net(name: str, seed: int = 0):
    from oracle import yolo_ref
    m, sd = model_and_weights(name, seed)
    net = yolo_ref.parse(m.yaml)
    fused = yolo_ref.fuse(net, sd)
    return net, fused


def fresh_model(name: str, seed: int = 0, fuse=True):
    """A new product Model instance loaded with the cached synthetic weights (fused like attempt_load)."""
    m0, sd = model_and_weights(name, seed)
    m = Model(name)
    m.load_state_dict(sd)
    m = m.float().eval()
    return m.fuse() if fuse else m


def frames(B, H, W, seed=1):
    return synthetic_frames(B, H, W, seed=seed)


def bordered(plan, t, B, H, W):
    """The whole NHWC tensor t of the last forward, zero frame included."""
    off, dims = ctypes.c_int64(), (ctypes.c_int64 * 4)()
    L.check(L.lib().yv7_tensor_info(plan._h, t, B, H, W, ctypes.byref(off), dims), 'yv7_tensor_info')
    dt = torch.float16 if plan.dtype == L.DT_F16 else torch.float32
    n = dims[0] * dims[1] * dims[2] * dims[3]
    return plan.workspace(B, H, W)[off.value:off.value + n * dt.itemsize].view(dt).view(*dims)
