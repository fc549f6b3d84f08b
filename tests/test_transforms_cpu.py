"""`not gpu` tests of the input transforms' host side (mmnn_sts_amd/transforms.py): the laws of every random draw, seeding,
the Gaussian taps, the zoom pad / crop geometry and the refusal of arguments upstream does not use."""
import math

import numpy as np
import pytest

from mmnn_sts_amd import transforms as T
from mmnn_sts_amd.utils.utils import Normalize

N_DRAWS = 4000


def _all_on(**kw):
    """train_transforms' stages with every prob replaced by `kw.get(name, 1.0)`."""
    p = lambda name: kw.get(name, 1.0)
    return T.Compose([T.EnsureChannelFirst(channel_dim=0), Normalize(286.9, 581.8), T.ScaleIntensity(),
                      T.RandRotate(range_x=15, prob=p("rot"), keep_size=True), T.RandAxisFlip(prob=p("flip")),
                      T.RandZoom(min_zoom=0.9, max_zoom=1.1, prob=p("zoom"), keep_size=True), T.Resize(spatial_size=T.SPATIAL_SIZE),
                      T.RandShiftIntensity(0.1, prob=p("shift")), T.RandAdjustContrast(prob=p("contrast")),
                      T.RandGaussianSmooth(prob=p("smooth")), T.RandGaussianSharpen(prob=p("sharpen")),
                      T.RandHistogramShift(prob=p("hist")), T.RandGaussianNoise(prob=p("noise"), mean=0, std=0.05), T.ToTensor()])


def test_draw_ranges_and_laws():
    ps = _all_on().set_random_state(7).randomize(N_DRAWS)
    th = np.array([p.theta for p in ps])
    assert th.min() >= -15.0 and th.max() <= 15.0 and th.min() < -14.0 and th.max() > 14.0      # radians, faithful to upstream
    z = np.array([p.zoom for p in ps])
    assert z.min() >= 0.9 and z.max() <= 1.1
    assert {p.flip_axis for p in ps} == {0, 1, 2}
    sh = np.array([p.shift for p in ps])
    assert sh.min() >= -0.1 and sh.max() <= 0.1
    g = np.array([p.gamma for p in ps])
    assert g.min() >= 0.5 and g.max() <= 4.5
    s = np.array([p.smooth_sigma for p in ps])
    assert s.min() >= 0.25 and s.max() <= 1.5 and abs(np.corrcoef(s[:, 0], s[:, 1])[0, 1]) < 0.1     # drawn independently per axis
    s1, s2 = np.array([p.sharpen_sigma1 for p in ps]), np.array([p.sharpen_sigma2 for p in ps])
    assert s1.min() >= 0.5 and s1.max() <= 1.0 and s2.min() >= 0.5 and np.all(s2 <= s1)
    a = np.array([p.alpha for p in ps])
    assert a.min() >= 10.0 and a.max() <= 30.0
    fl = np.array([p.hist_fl for p in ps])
    assert np.all(fl[:, 0] == 0.0) and np.all(fl[:, -1] == 1.0) and np.all(np.diff(fl, axis=1) >= 0.0)
    ns = np.array([p.noise_std for p in ps])
    assert ns.min() >= 0.0 and ns.max() <= 0.05
    assert len({p.noise_seed for p in ps}) == N_DRAWS


def test_gating_frequencies_are_binomial():
    tf = T.train_transforms
    rng_tf = T.Compose(tf.transforms).set_random_state(11)
    ps = rng_tf.randomize(N_DRAWS)
    for bit, prob in ((T.ROTATE, 0.5), (T.FLIP, 0.5), (T.ZOOM, 0.5), (T.SHIFT, 0.3), (T.CONTRAST, 0.3), (T.SMOOTH, 0.2), (T.SHARPEN, 0.2),
                      (T.HIST, 0.3), (T.NOISE, 0.3)):
        k = sum(1 for p in ps if p.fire & bit)
        sd = math.sqrt(N_DRAWS * prob * (1 - prob))
        assert abs(k - N_DRAWS * prob) <= 4 * sd, (bit, k)
    assert not any(p.fire & (T.NORMALIZE | T.SCALE | T.RESIZE) for p in ps)


def test_val_transforms_draw_nothing():
    assert all(p.fire == 0 for p in T.val_transforms.randomize(16))
    assert T.val_transforms.stages == T.NORMALIZE | T.SCALE | T.RESIZE
    assert T.train_transforms.stages == (1 << 12) - 1


def test_set_random_state_reproduces():
    a = _all_on(rot=0.5, zoom=0.5, noise=0.3).set_random_state(123).randomize(64)
    b = _all_on(rot=0.5, zoom=0.5, noise=0.3).set_random_state(123).randomize(64)
    c = _all_on(rot=0.5, zoom=0.5, noise=0.3).set_random_state(124).randomize(64)
    assert a == b and a != c


def test_default_seed_follows_torch_seed():
    import torch
    torch.manual_seed(5)
    s1 = T._default_seed()
    torch.manual_seed(6)
    s2 = T._default_seed()
    assert s1 != s2


@pytest.mark.parametrize("sigma,length", [(0.25, 3), (1.0, 9), (1.5, 13)])
def test_gaussian_taps(sigma, length):
    k = T.gaussian_taps(sigma)
    assert len(k) == length
    t = length // 2
    ref = [0.5 * (math.erf((i + 0.5) / (sigma * math.sqrt(2))) - math.erf((i - 0.5) / (sigma * math.sqrt(2)))) for i in range(-t, t + 1)]
    np.testing.assert_allclose(k, ref, rtol=0, atol=1e-15)
    assert np.allclose(k, k[::-1]) and k.sum() < 1.0 + 1e-12      # symmetric, not renormalised
    assert len(T.gaussian_taps(1.5)) <= T.MAX_TAPS


@pytest.mark.parametrize("n,z,m,off", [
    (64, 0.9, 57, -3),        # m < n, n - m odd: 3 before, 4 after
    (64, 0.95, 60, -2),       # m < n, even difference
    (63, 0.9, 56, -3),        # odd n
    (64, 1.1, 70, 3),         # m > n: crop from m // 2 - n // 2
    (63, 1.1, 69, 3),         # 34 - 31
    (37, 1.05, 38, 1),        # 19 - 18
    (50, 1.0, 50, 0),
])
def test_zoom_geometry(n, z, m, off):
    assert T.zoom_geometry(n, z) == (m, off)


def test_zoom_geometry_pad_split():
    for n in range(20, 140):
        for z in (0.9, 0.93, 0.97):
            m, off = T.zoom_geometry(n, z)
            before = -off
            assert m == math.floor(n * z) and before == (n - m) // 2 and (n - m) - before >= before


@pytest.mark.parametrize("make", [
    lambda: T.RandRotate(range_x=10, prob=0.5),
    lambda: T.RandRotate(range_x=15, prob=0.5, keep_size=False),
    lambda: T.RandRotate(range_x=15, range_y=5, prob=0.5),
    lambda: T.RandZoom(min_zoom=0.8, max_zoom=1.1, prob=0.5),
    lambda: T.RandZoom(prob=0.5, keep_size=False),
    lambda: T.Resize(spatial_size=(96, 96, 96)),
    lambda: T.Resize(spatial_size=T.SPATIAL_SIZE, mode="trilinear"),
    lambda: T.RandShiftIntensity(0.2, prob=0.3),
    lambda: T.RandAdjustContrast(prob=0.3, gamma=(0.7, 1.5)),
    lambda: T.RandGaussianSmooth(sigma_x=(0.5, 1.0), prob=0.2),
    lambda: T.RandGaussianSharpen(alpha=(5.0, 10.0), prob=0.2),
    lambda: T.RandHistogramShift(num_control_points=5, prob=0.3),
    lambda: T.RandGaussianNoise(prob=0.3, mean=0, std=0.1),
    lambda: T.RandGaussianNoise(prob=0.3, mean=1.0, std=0.05),
    lambda: T.ScaleIntensity(minv=-1.0, maxv=1.0),
    lambda: T.EnsureChannelFirst(channel_dim=-1),
    lambda: T.RandAxisFlip(prob=1.5),
    lambda: Normalize(0.0, 0.0),
])
def test_unsupported_arguments_are_rejected(make):
    with pytest.raises(ValueError):
        make()


def test_compose_rejects_wrong_order_and_repeats():
    with pytest.raises(ValueError):
        T.Compose([T.Resize(), T.RandZoom(prob=0.5)])
    with pytest.raises(ValueError):
        T.Compose([T.ScaleIntensity(), T.ScaleIntensity()])
    with pytest.raises(ValueError):
        T.Compose([object()])


def test_upstream_pipelines_built_as_in_main():
    names = [type(t).__name__ for t in T.train_transforms.transforms]
    assert names == ["EnsureChannelFirst", "Normalize", "ScaleIntensity", "RandRotate", "RandAxisFlip", "RandZoom", "Resize",
                     "RandShiftIntensity", "RandAdjustContrast", "RandGaussianSmooth", "RandGaussianSharpen", "RandHistogramShift",
                     "RandGaussianNoise", "ToTensor"]
    assert [type(t).__name__ for t in T.val_transforms.transforms] == ["EnsureChannelFirst", "Normalize", "ScaleIntensity", "Resize", "ToTensor"]
    assert T.SPATIAL_SIZE == (64, 64, 64) and T.train_transforms.norm == (286.90859071507913, 581.7816096485366)
    probs = [getattr(t, "prob", None) for t in T.train_transforms.transforms]
    assert probs == [None, None, None, 0.5, 0.5, 0.5, None, 0.3, 0.3, 0.2, 0.2, 0.3, 0.3, None]


def test_param_record_layout():
    """The ctypes mirror of mmnn_transform_params packs the taps and the zoom geometry the kernels index with."""
    import ctypes
    from mmnn_sts_amd import _lib
    rec = _lib.TransformParams()
    p = T.SampleParams(fire=T.ZOOM | T.SMOOTH | T.NOISE, zoom=0.9, smooth_sigma=(0.25, 1.0, 1.5), noise_seed=(1 << 63) + 5)
    T.train_transforms._pack(p, (64, 37, 50), rec)
    assert list(rec.zoom_m) == [57, 33, 45] and list(rec.zoom_off) == [-3, -2, -2]
    assert list(rec.smooth_r) == [1, 4, 6]
    np.testing.assert_allclose(list(rec.smooth_k[2]), T.gaussian_taps(1.5), rtol=1e-7)
    assert rec.noise_seed == (1 << 63) + 5
    assert ctypes.sizeof(_lib.TransformParams) % 8 == 0 and _lib.TransformParams.theta.offset == 8
