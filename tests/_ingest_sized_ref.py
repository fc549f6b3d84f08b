"""Helper of the size-S ingest tests: the fp64 restatements of the two `_sized` contracts of include/mmnn_sts.h, built from the
parametrised pieces of tests/_ingest_ref.py (`masked_volume`, `area_resize_fp64(v, size)`) and tests/_scan_space_ref.py (`taps(m, size)`).
At size 64 they reproduce `_ingest_ref.ingest_ref` and `_scan_space_ref.maps_to_scan_ref` bit for bit (asserted in
tests/test_ingest_size_cpu.py).  The bounds are those files' own and do not depend on S.  Shares no code with mmnn_sts_amd."""
import numpy as np

from tests import _ingest_ref as R
from tests import _scan_space_ref as S

MAX_SIZE = 128


def ingest_ref(scan, mask, size=R.SIZE, scan_scaling=(1.0, 0.0), mask_scaling=(1.0, 0.0)):
    """(plane float64 (size,) * 3, extents (Mx, My, Mz), v): image * mask in float64, every all-zero slice dropped along each axis (NaN
    counts as non-zero), area resize to size^3.  An empty result -> zeros and (0, 0, 0)."""
    with np.errstate(invalid="ignore", over="ignore"):
        v = R.masked_volume(scan, mask, scan_scaling, mask_scaling)
        keep = S.keep_flags_of(v)
        ext = tuple(int(k.sum()) for k in keep)
        if min(ext) == 0:
            return np.zeros((size,) * 3), (0, 0, 0), v
        return R.area_resize_fp64(v[keep[0]][:, keep[1]][:, :, keep[2]], size), ext, v


def upsample(vol, ext):
    """`vol` (size,) * 3 -> (Mx, My, Mz) float64 by the tap rule with S = size, one axis after the other."""
    v = np.asarray(vol, dtype=np.float64)
    size = v.shape[0]
    assert v.shape == (size,) * 3
    for axis, m in enumerate(ext):
        i0, i1, w = S.taps(m, size)
        w = w.reshape([m if a == axis else 1 for a in range(3)])
        v = (1.0 - w) * v.take(i0, axis=axis) + w * v.take(i1, axis=axis)
    return v


def maps_to_scan_ref(maps, keep):
    """maps (n, size, size, size) -> (n, x, y, z) float64 on the scan's grid: zeros where a slice is dropped (or an axis keeps nothing)."""
    maps = np.asarray(maps, dtype=np.float64)
    ext = tuple(int(k.sum()) for k in keep)
    out = np.zeros((maps.shape[0],) + tuple(len(k) for k in keep), dtype=np.float64)
    if min(ext) == 0:
        return out
    ix = np.ix_(*[np.flatnonzero(k) for k in keep])
    for n in range(maps.shape[0]):
        out[n][ix] = upsample(maps[n], ext)
    return out
