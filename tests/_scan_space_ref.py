"""Helper of the scan-space tests: the fp64 numpy restatement of the `mmnn_maps_to_scan` contract (include/mmnn_sts.h) -- a 64^3 map of
the model, up-sampled trilinearly (align_corners=False) to the extents the ingest kept and scattered to the kept positions of the scan's
grid, zeros on every dropped slice.  The kept slices are the keep flags of `tests/_ingest_ref.py:ingest_ref`'s masked volume.  Shares no
code with mmnn_sts_amd."""
import numpy as np

from tests import _ingest_ref as R

SIZE = 64


def taps(m, size=SIZE):
    """(i0, i1, w) of the m kept positions of one axis: s = max((p + 0.5) size / m - 0.5, 0), i0 = min(floor(s), size - 1),
    i1 = min(i0 + 1, size - 1), w = s - i0, all in float64."""
    p = np.arange(m, dtype=np.float64)
    s = np.maximum((p + 0.5) * float(size) / float(m) - 0.5, 0.0)
    i0 = np.minimum(np.floor(s).astype(np.int64), size - 1)
    i1 = np.minimum(i0 + 1, size - 1)
    return i0, i1, s - i0.astype(np.float64)


def upsample(vol, ext):
    """`vol` (S, S, S) -> (Mx, My, Mz) float64: the separable blend with weights 1 - w, w along each axis."""
    v = np.asarray(vol, dtype=np.float64)
    for axis, m in enumerate(ext):
        i0, i1, w = taps(m, v.shape[axis])
        shape = [1, 1, 1]
        shape[axis] = m
        w = w.reshape(shape)
        v = (1.0 - w) * v.take(i0, axis=axis) + w * v.take(i1, axis=axis)
    return v


def keep_flags_of(v):
    """Per axis the boolean keep flags of the slices of the masked volume `v` (the third value of `ingest_ref`), by its rule: a slice is
    kept when any of its voxels has not (v == 0); NaN counts as non-zero."""
    with np.errstate(invalid="ignore"):
        nz = ~(v == 0)
    return [np.any(nz, axis=tuple(a for a in range(3) if a != axis)) for axis in range(3)]


def keep_flags(scan, mask, scan_scaling=(1.0, 0.0), mask_scaling=(1.0, 0.0)):
    return keep_flags_of(R.masked_volume(scan, mask, scan_scaling, mask_scaling))


def maps_to_scan_ref(maps, keep):
    """maps (n, S, S, S) -> (n, x, y, z) float64 on the scan's grid: zeros where a slice is dropped (or when an axis keeps nothing)."""
    maps = np.asarray(maps, dtype=np.float64)
    ext = tuple(int(k.sum()) for k in keep)
    out = np.zeros((maps.shape[0],) + tuple(len(k) for k in keep), dtype=np.float64)
    if min(ext) == 0:
        return out
    ix = np.ix_(*[np.flatnonzero(k) for k in keep])
    for n in range(maps.shape[0]):
        out[n][ix] = upsample(maps[n], ext)
    return out


def tolerance(maps):
    """2 * 2^-24 * max|map|: the device forms the blend in fp64, so its one visible error is the final rounding to fp32 of a value of
    magnitude at most max|map| (a convex combination) -- half a unit; two units are allowed, the convention of `_ingest_ref.tolerance`."""
    return 2.0 * 2.0 ** -24 * float(np.abs(np.asarray(maps, dtype=np.float64)).max())
