"""Shared helpers for the tests: synthetic state dicts / inputs identical to oracle/make_golden.py."""
import os

import numpy as np
import torch

from oracle import synth
from oracle import restatement as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N_CLIN = 32


def load_golden(name):
    return np.load(os.path.join(GOLDEN, name), allow_pickle=False)


def synth_sd(schema, prefix, device="cpu", requires_grad=False):
    sd = {}
    for k, v in synth.synth_state_dict(schema, prefix).items():
        t = torch.from_numpy(np.asarray(v)).to(device)
        if requires_grad and t.is_floating_point() and "running" not in k:
            t.requires_grad_(True)
        sd[k] = t
    return sd


def image_in(n, c, s):
    return torch.from_numpy(synth.uniform(f"image/{n}x{c}x{s}", (n, c, s, s, s)))


def clin_in(n):
    return torch.from_numpy(synth.uniform(f"clinical/{n}", (n, N_CLIN)))


def labels(n):
    if n == 2:
        ev = np.array([[1, 0], [0, 1]], dtype=np.int64)
        du = np.array([[100, 250], [300, 50]], dtype=np.int64)
    else:
        ev = (synth.uniform(f"events/{n}", (n, 2)) > 0).astype(np.int64)
        ev[0, :] = 1
        du = (1 + np.floor((synth.uniform(f"durations/{n}", (n, 2)) * 0.5 + 0.5) * 2998)).astype(np.int64)
    return torch.from_numpy(ev), torch.from_numpy(du)


def stat3(t):
    t = t.detach().double().cpu()
    return np.array([t.mean().item(), t.abs().mean().item(), t.abs().max().item()])


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


# --------------------------------------------------------------------------------------------------------------
# Dropout masks of the device, restated (csrc/common.hpp: drop_scale; csrc/tail.hip / csrc/resnet.hip: the element-wise
# keyings).  Pure functions of (seed, key, p): numpy uint64 arithmetic wraps modulo 2^64 like the device's.  Pinned by
# tests/test_dropout_cpu.py (statistics, independence) and by the masks read off the device (tests/test_backbone_gpu.py).
# --------------------------------------------------------------------------------------------------------------
_GOLD = np.uint64(0x9E3779B97F4A7C15)
_ELEM_K = np.uint64(0xD1B54A32D192ED03)
MLP_DROP_LAYER0 = 0x7E0000
FEAT_DROP_LAYER0 = 0x7F0000


def _mix64(x):
    """splitmix64 finaliser of a uint64 array (the increment included)."""
    with np.errstate(over="ignore"):
        x = x + _GOLD
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def _scale_of_bits(x, p):
    """24 top bits -> uniform fp32 in [0, 1); u < p ? 0 : 1 / (1 - p), every step in fp32."""
    p32 = np.float32(p)
    u = (x >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    keep = np.float32(1.0) / (np.float32(1.0) - p32)
    return np.where(u < p32, np.float32(0.0), keep).astype(np.float32)


def _seed64(seed):
    seed = int(seed)
    assert 0 <= seed < 2 ** 64
    return np.uint64(seed)


def drop_scale_ref(seed, layer, n, c, p):
    """Keep-scale of channel `c` of sample `n` in layer `layer` (layer, n, c: integers or arrays, broadcast): 0 or 1/(1-p), fp32."""
    layer, n, c = np.broadcast_arrays(np.asarray(layer, dtype=np.int64), np.asarray(n, dtype=np.int64), np.asarray(c, dtype=np.int64))
    if p <= 0.0:
        return np.ones(n.shape, dtype=np.float32)
    m32 = np.int64(0xFFFFFFFF)
    key = (((layer & m32).astype(np.uint64) << np.uint64(40)) ^ ((n & m32).astype(np.uint64) << np.uint64(20))
           ^ (c & m32).astype(np.uint64))
    with np.errstate(over="ignore"):
        x = _seed64(seed) + _GOLD * key
    return _scale_of_bits(_mix64(x), p)


def channel_drop_mask(seed, layer, n, channels, p):
    """(n, channels) mask of a dense layer's Dropout3d (layer: 0-based over all dense layers in module order)."""
    return drop_scale_ref(seed, layer, np.arange(n)[:, None], np.arange(channels)[None, :], p)


def backbone_drop_masks(cfg, seed, n, p):
    """{"b{b}l{l}": (n, growth) torch fp64 mask} for oracle.restatement.densenet_backbone(drop_masks=)."""
    masks, layer = {}, 0
    for b, nl in enumerate(cfg.block_config, start=1):
        for l in range(1, nl + 1):
            masks[f"b{b}l{l}"] = torch.from_numpy(channel_drop_mask(seed, layer, n, cfg.growth_rate, p)).double()
            layer += 1
    return masks


def feat_drop_mask_ref(seed, n, f, p):
    """(n, f) element mask of DenseNet.features (csrc/tail.hip: the flat index n*f + j packed into layer / sample / channel)."""
    idx = np.arange(n * f, dtype=np.int64)
    return drop_scale_ref(seed, FEAT_DROP_LAYER0 + (idx >> 20), (idx >> 10) & 1023, idx & 1023, p).reshape(n, f)


def mlp_row_mask_ref(seed, layer, n, p):
    """(n,) row mask of MLP layer `layer` (= first_layer_id + index inside the stack)."""
    return drop_scale_ref(seed, MLP_DROP_LAYER0 + layer, np.arange(n), 0, p)


def resnet_elem_mask_ref(seed, count, p):
    """(count,) element mask of BatchNormAct3d (csrc/resnet.hip: mix64(seed ^ K * (idx + 1)))."""
    if p <= 0.0:
        return np.ones(count, dtype=np.float32)
    with np.errstate(over="ignore"):
        x = _seed64(seed) ^ (_ELEM_K * (np.arange(count, dtype=np.uint64) + np.uint64(1)))
    return _scale_of_bits(_mix64(x), p)
