"""Upstream's input transforms (main.py:64-92: `train_transforms`, `val_transforms`) on the MI355X.

The classes carry monai's names and upstream's arguments; only the argument values upstream uses are supported, anything else
raises ValueError.  The semantics are pinned by the table in DESIGN §11 (a restatement of monai 1.x with upstream's arguments;
monai itself is not a dependency).  Work is split in two:

  * `Compose.randomize(n)`: host code, every random draw of the batch from a `numpy.random.Generator`.  Draw order: sample by
    sample; within a sample, stage by stage in pipeline order; within a random stage, first the gate `U[0,1) < prob`, then (only
    when it fires) the stage's parameters in the order the table lists them.
  * `Compose.apply(x, params)`: ONE native call (`mmnn_transform_volumes`, csrc/transforms.hip) for the whole batch.

`Compose(x)` is `apply(x, randomize(N))`; a transform called on its own behaves as a one-element Compose.  Inputs are CUDA fp32
tensors of shape (N, C, D, H, W) or (C, D, H, W); the result is a new tensor.

`pipelines(size)` returns upstream's two pipelines with the Resize target (size,) * 3 -- the one departure from upstream's argument
values, for runs whose volumes are ingested at another extent than 64 (`--image_size`).  `train_transforms` / `val_transforms` are
`pipelines(64)`; the public `Resize(spatial_size=...)` still admits upstream's value only.
"""
import ctypes
import math
import os
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import _lib
from .data.constants import IMAGE_DATA_MEAN, IMAGE_DATA_STDDEV
from .utils.utils import Normalize

SPATIAL_SIZE = (64, 64, 64)      # main.py:60
MAX_SIZE = 128                   # the largest Resize target of `pipelines` (MMNN_INGEST_MAX_SIZE: what the scan ingest can feed)

# stage bits, in pipeline order (include/mmnn_sts.h: MMNN_TF_*)
NORMALIZE, SCALE, ROTATE, FLIP, ZOOM, RESIZE, SHIFT, CONTRAST, SMOOTH, SHARPEN, HIST, NOISE = (1 << i for i in range(12))
MAX_TAPS = _lib.TF_MAX_TAPS


# ---- host-side derivations (unit-tested on CPU) --------------------------------------------------------------------------------
def gaussian_taps(sigma: float) -> np.ndarray:
    """1-D taps k[-t..t] of the 'erf' Gaussian: k[i] = (erf((i+1/2)/(sigma sqrt 2)) - erf((i-1/2)/(sigma sqrt 2))) / 2,
    t = int(max(4 sigma, 0.5) + 0.5), not renormalised."""
    t = int(max(4.0 * sigma, 0.5) + 0.5)
    s = sigma * math.sqrt(2.0)
    return np.array([0.5 * (math.erf((i + 0.5) / s) - math.erf((i - 0.5) / s)) for i in range(-t, t + 1)], dtype=np.float64)


def zoom_geometry(n: int, z: float) -> Tuple[int, int]:
    """RandZoom along one axis of extent n: the area-resized extent m = floor(n z) and the offset `off` with which output index o
    reads resized index clamp(o + off, 0, m - 1): edge padding with (n - m) // 2 before when m < n, a crop starting at
    m // 2 - n // 2 when m > n."""
    m = int(math.floor(n * z))
    if m < n:
        return m, -((n - m) // 2)
    if m > n:
        return m, m // 2 - n // 2
    return m, 0


@dataclass
class SampleParams:
    """The draws of one sample.  `fire`: stage bits of the random stages that apply to it."""
    fire: int = 0
    theta: float = 0.0
    flip_axis: int = 0
    zoom: float = 1.0
    shift: float = 0.0
    gamma: float = 1.0
    smooth_sigma: Tuple[float, float, float] = (1.0, 1.0, 1.0)
    sharpen_sigma1: Tuple[float, float, float] = (1.0, 1.0, 1.0)
    sharpen_sigma2: Tuple[float, float, float] = (0.5, 0.5, 0.5)
    alpha: float = 10.0
    hist_fl: Tuple[float, ...] = field(default_factory=lambda: tuple(np.linspace(0.0, 1.0, 10)))
    noise_std: float = 0.0
    noise_seed: int = 0


_seeded = [0]


def _default_seed() -> int:
    """As ops.next_seed: from torch's seed (so `torch.manual_seed` makes runs repeat), a per-object counter and the rank."""
    _seeded[0] += 1
    rank = int(os.environ.get("RANK", "0") or 0)
    return (torch.initial_seed() * 0x9E3779B97F4A7C15 + _seeded[0] * 0x5851F42D4C957F2D + rank * 0xA24BAED4963EE407) & 0xFFFFFFFFFFFFFFFF


def _reject(name, what, value, allowed):
    raise ValueError(f"{name}: {what}={value!r} is not supported (only {allowed!r}, the value upstream's main.py uses)")


def _check_prob(name, prob):
    if not 0.0 <= float(prob) <= 1.0:
        raise ValueError(f"{name}: prob={prob!r} outside [0, 1]")
    return float(prob)


class Transform:
    """One stage.  `bit` = 0 for the no-op stages; `prob` is None for the deterministic ones."""
    bit = 0
    prob: Optional[float] = None

    def draw(self, rng: np.random.Generator, p: SampleParams) -> None:
        if self.prob is None:
            return
        if rng.random() < self.prob:
            p.fire |= self.bit
            self.draw_params(rng, p)

    def draw_params(self, rng, p):
        pass

    def set_random_state(self, seed=None):
        self._rng = np.random.default_rng(seed)
        return self

    def __call__(self, x):
        c = Compose([self])
        if getattr(self, "_rng", None) is None:
            self._rng = np.random.default_rng(_default_seed())
        c._rng = self._rng
        return c(x)


class EnsureChannelFirst(Transform):
    def __init__(self, channel_dim=0):
        if channel_dim != 0:
            _reject("EnsureChannelFirst", "channel_dim", channel_dim, 0)


class ToTensor(Transform):
    pass


class ScaleIntensity(Transform):
    bit = SCALE

    def __init__(self, minv=0.0, maxv=1.0):
        if (minv, maxv) != (0.0, 1.0):
            _reject("ScaleIntensity", "(minv, maxv)", (minv, maxv), (0.0, 1.0))


class RandRotate(Transform):
    """theta ~ U(-range_x, range_x) in RADIANS: upstream passes 15 to monai's radians argument; kept faithful."""
    bit = ROTATE

    def __init__(self, range_x=15, range_y=0.0, range_z=0.0, prob=0.1, keep_size=True, mode="bilinear", padding_mode="border"):
        for what, v, ok in (("range_x", range_x, 15), ("range_y", range_y, 0.0), ("range_z", range_z, 0.0), ("keep_size", keep_size, True),
                            ("mode", mode, "bilinear"), ("padding_mode", padding_mode, "border")):
            if v != ok:
                _reject("RandRotate", what, v, ok)
        self.range_x = float(range_x)
        self.prob = _check_prob("RandRotate", prob)

    def draw_params(self, rng, p):
        p.theta = float(rng.uniform(-self.range_x, self.range_x))


class RandAxisFlip(Transform):
    bit = FLIP

    def __init__(self, prob=0.1):
        self.prob = _check_prob("RandAxisFlip", prob)

    def draw_params(self, rng, p):
        p.flip_axis = int(rng.integers(3))


class RandZoom(Transform):
    bit = ZOOM

    def __init__(self, min_zoom=0.9, max_zoom=1.1, prob=0.1, keep_size=True, mode="area", padding_mode="edge"):
        for what, v, ok in (("min_zoom", min_zoom, 0.9), ("max_zoom", max_zoom, 1.1), ("keep_size", keep_size, True), ("mode", mode, "area"),
                            ("padding_mode", padding_mode, "edge")):
            if v != ok:
                _reject("RandZoom", what, v, ok)
        self.min_zoom, self.max_zoom = float(min_zoom), float(max_zoom)
        self.prob = _check_prob("RandZoom", prob)

    def draw_params(self, rng, p):
        p.zoom = float(rng.uniform(self.min_zoom, self.max_zoom))


class Resize(Transform):
    bit = RESIZE

    def __init__(self, spatial_size=SPATIAL_SIZE, mode="area"):
        size = tuple(int(s) for s in spatial_size) if hasattr(spatial_size, "__len__") else (int(spatial_size),) * 3
        if size != tuple(SPATIAL_SIZE):
            _reject("Resize", "spatial_size", spatial_size, SPATIAL_SIZE)
        if mode != "area":
            _reject("Resize", "mode", mode, "area")
        self.spatial_size = size

    @classmethod
    def _sized(cls, size: int) -> "Resize":
        """The Resize of `pipelines(size)`: target (size,) * 3 with size in 1..MAX_SIZE.  Not part of the public surface."""
        if isinstance(size, bool) or not isinstance(size, (int, np.integer)) or not 1 <= int(size) <= MAX_SIZE:
            raise ValueError(f"pipelines: size={size!r} is not an integer in 1..{MAX_SIZE}")
        t = cls()
        t.spatial_size = (int(size),) * 3
        return t


class RandShiftIntensity(Transform):
    bit = SHIFT

    def __init__(self, offsets=0.1, prob=0.1):
        if offsets not in (0.1, (-0.1, 0.1)):
            _reject("RandShiftIntensity", "offsets", offsets, 0.1)
        self.prob = _check_prob("RandShiftIntensity", prob)

    def draw_params(self, rng, p):
        p.shift = float(rng.uniform(-0.1, 0.1))


class RandAdjustContrast(Transform):
    bit = CONTRAST

    def __init__(self, prob=0.1, gamma=(0.5, 4.5)):
        if tuple(gamma) != (0.5, 4.5):
            _reject("RandAdjustContrast", "gamma", gamma, (0.5, 4.5))
        self.prob = _check_prob("RandAdjustContrast", prob)

    def draw_params(self, rng, p):
        p.gamma = float(rng.uniform(0.5, 4.5))


class RandGaussianSmooth(Transform):
    bit = SMOOTH

    def __init__(self, sigma_x=(0.25, 1.5), sigma_y=(0.25, 1.5), sigma_z=(0.25, 1.5), prob=0.1, approx="erf"):
        for what, v, ok in (("sigma_x", tuple(sigma_x), (0.25, 1.5)), ("sigma_y", tuple(sigma_y), (0.25, 1.5)),
                            ("sigma_z", tuple(sigma_z), (0.25, 1.5)), ("approx", approx, "erf")):
            if v != ok:
                _reject("RandGaussianSmooth", what, v, ok)
        self.prob = _check_prob("RandGaussianSmooth", prob)

    def draw_params(self, rng, p):
        p.smooth_sigma = tuple(float(rng.uniform(0.25, 1.5)) for _ in range(3))


class RandGaussianSharpen(Transform):
    bit = SHARPEN

    def __init__(self, sigma1_x=(0.5, 1.0), sigma1_y=(0.5, 1.0), sigma1_z=(0.5, 1.0), sigma2_x=0.5, sigma2_y=0.5, sigma2_z=0.5,
                 alpha=(10.0, 30.0), approx="erf", prob=0.1):
        for what, v, ok in (("sigma1_x", tuple(sigma1_x), (0.5, 1.0)), ("sigma1_y", tuple(sigma1_y), (0.5, 1.0)),
                            ("sigma1_z", tuple(sigma1_z), (0.5, 1.0)), ("sigma2_x", sigma2_x, 0.5), ("sigma2_y", sigma2_y, 0.5),
                            ("sigma2_z", sigma2_z, 0.5), ("alpha", tuple(alpha), (10.0, 30.0)), ("approx", approx, "erf")):
            if v != ok:
                _reject("RandGaussianSharpen", what, v, ok)
        self.prob = _check_prob("RandGaussianSharpen", prob)

    def draw_params(self, rng, p):
        s1 = tuple(float(rng.uniform(0.5, 1.0)) for _ in range(3))
        p.sharpen_sigma1 = s1
        p.sharpen_sigma2 = tuple(float(rng.uniform(0.5, s)) for s in s1)
        p.alpha = float(rng.uniform(10.0, 30.0))


class RandHistogramShift(Transform):
    bit = HIST

    def __init__(self, num_control_points=10, prob=0.1):
        if num_control_points != 10:
            _reject("RandHistogramShift", "num_control_points", num_control_points, 10)
        self.prob = _check_prob("RandHistogramShift", prob)

    def draw_params(self, rng, p):
        fl = np.linspace(0.0, 1.0, 10)
        for i in range(1, 9):
            fl[i] = rng.uniform(fl[i - 1], fl[i + 1])
        p.hist_fl = tuple(float(v) for v in fl)


class RandGaussianNoise(Transform):
    bit = NOISE

    def __init__(self, prob=0.1, mean=0.0, std=0.05):
        if mean != 0:
            _reject("RandGaussianNoise", "mean", mean, 0)
        if std != 0.05:
            _reject("RandGaussianNoise", "std", std, 0.05)
        self.std = float(std)
        self.prob = _check_prob("RandGaussianNoise", prob)

    def draw_params(self, rng, p):
        p.noise_std = float(rng.uniform(0.0, self.std))
        p.noise_seed = int(rng.integers(0, 1 << 63))


class Compose:
    """A pipeline of the stages above (and utils.Normalize) in upstream's order; each stage at most once."""

    def __init__(self, transforms):
        self.transforms = list(transforms)
        self.stages = 0
        self.norm = (0.0, 1.0)
        self.spatial_size = None
        last = 0
        for t in self.transforms:
            bit = getattr(t, "bit", None)
            if bit is None:
                raise ValueError(f"Compose: {type(t).__name__} is not one of the supported transforms")
            if bit == 0:
                continue
            if bit <= last:
                raise ValueError(f"Compose: {type(t).__name__} out of upstream's order (main.py:64-92) or repeated")
            last = bit
            self.stages |= bit
            if bit == NORMALIZE:
                self.norm = (float(t.mean), float(t.stddev))
            if bit == RESIZE:
                self.spatial_size = t.spatial_size
        self._rng = None

    def set_random_state(self, seed=None):
        self._rng = np.random.default_rng(seed)
        return self

    def randomize(self, n: int) -> List[SampleParams]:
        if self._rng is None:
            self._rng = np.random.default_rng(_default_seed())
        out = []
        for _ in range(n):
            p = SampleParams()
            for t in self.transforms:
                if getattr(t, "prob", None) is not None:
                    t.draw(self._rng, p)
            out.append(p)
        return out

    def _pack(self, p: SampleParams, ext, rec) -> None:
        rec.fire = p.fire & self.stages
        rec.flip_axis = int(p.flip_axis)
        rec.theta = float(p.theta)
        rec.noise_seed = int(p.noise_seed) & 0xFFFFFFFFFFFFFFFF
        for k in range(3):
            rec.zoom_m[k], rec.zoom_off[k] = zoom_geometry(ext[k], p.zoom)
        rec.shift, rec.gamma, rec.alpha, rec.noise_std = p.shift, p.gamma, p.alpha, p.noise_std
        if len(p.hist_fl) != 10:
            raise ValueError("hist_fl needs 10 control points")
        for k, v in enumerate(p.hist_fl):
            rec.hist_fl[k] = v
        for bit, radius, taps, sig in ((SMOOTH, rec.smooth_r, rec.smooth_k, p.smooth_sigma), (SHARPEN, rec.sharp1_r, rec.sharp1_k, p.sharpen_sigma1),
                                       (SHARPEN, rec.sharp2_r, rec.sharp2_k, p.sharpen_sigma2)):
            if not rec.fire & bit:
                continue
            for k in range(3):
                tp = gaussian_taps(sig[k])
                if len(tp) > MAX_TAPS:
                    raise ValueError(f"Gaussian sigma {sig[k]} needs {len(tp)} taps (at most {MAX_TAPS})")
                radius[k] = len(tp) // 2
                for j, v in enumerate(tp):
                    taps[k][j] = v

    def apply(self, x: torch.Tensor, params: List[SampleParams]) -> torch.Tensor:
        single = x.dim() == 4
        if single:
            x = x.unsqueeze(0)
        if x.dim() != 5 or not x.is_cuda or x.dtype != torch.float32:
            raise ValueError(f"transforms: expected a CUDA float32 tensor of shape (N, C, D, H, W) or (C, D, H, W), got "
                             f"{tuple(x.shape)} {x.dtype} on {x.device}")
        x = x.contiguous()
        n, c, d, h, w = x.shape
        if len(params) != n:
            raise ValueError(f"transforms: {len(params)} parameter records for a batch of {n}")
        od, oh, ow = self.spatial_size if self.stages & RESIZE else (d, h, w)
        desc = _lib.TransformDesc(n, c, d, h, w, od, oh, ow, self.stages, self.norm[0], self.norm[1])
        recs = (_lib.TransformParams * n)()
        for i, p in enumerate(params):
            self._pack(p, (d, h, w), recs[i])
        nbytes = _lib.count("mmnn_transform_workspace_bytes", ctypes.byref(desc))
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=x.device)
        if os.environ.get("MMNN_POISON_WS") == "1":   # debugging aid: NaN-fill so reads of unwritten workspace words surface
            ws.fill_(255)
        out = torch.empty((n, c, od, oh, ow), dtype=torch.float32, device=x.device)
        _lib.enqueue("mmnn_transform_volumes", ctypes.byref(desc), recs, x.data_ptr(), out.data_ptr(), ws.data_ptr(), nbytes, device=x.device)
        return out[0] if single else out

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        return self.apply(x, self.randomize(x.shape[0] if x.dim() == 5 else 1))


def pipelines(size: int = SPATIAL_SIZE[0]) -> Tuple[Compose, Compose]:
    """(train, val): upstream's two pipelines (main.py:64-92) with the Resize target (size,) * 3, size in 1..MAX_SIZE.  Every other
    argument is upstream's, so the stages, their order and the draws of `randomize` do not depend on `size`."""
    train = Compose([
        EnsureChannelFirst(channel_dim=0),
        Normalize(IMAGE_DATA_MEAN, IMAGE_DATA_STDDEV),
        ScaleIntensity(),
        # spatial
        RandRotate(range_x=15, prob=0.5, keep_size=True),
        RandAxisFlip(prob=0.5),
        RandZoom(min_zoom=0.9, max_zoom=1.1, prob=0.5, keep_size=True),
        Resize._sized(size),
        # intensity
        RandShiftIntensity(0.1, prob=0.3),
        RandAdjustContrast(prob=0.3),
        RandGaussianSmooth(prob=0.2),
        RandGaussianSharpen(prob=0.2),
        RandHistogramShift(prob=0.3),
        RandGaussianNoise(prob=0.3, mean=0, std=0.05),
        ToTensor(),
    ])
    val = Compose([
        EnsureChannelFirst(channel_dim=0),
        Normalize(IMAGE_DATA_MEAN, IMAGE_DATA_STDDEV),
        ScaleIntensity(),
        Resize._sized(size),
        ToTensor(),
    ])
    return train, val


train_transforms, val_transforms = pipelines(SPATIAL_SIZE[0])
