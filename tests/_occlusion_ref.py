"""Numpy restatement of the occlusion-sensitivity contract (the comment above mmnn_occlusion_window_count in include/mmnn_sts.h): the
window grid, the occluded batch and the map with its fp64 order.  Written from the contract; it shares no code with the package, and it
finds the covering windows of a voxel by testing every window, not by a formula."""
import numpy as np


def triple(v):
    return tuple(int(t) for t in v) if isinstance(v, (tuple, list)) else (int(v),) * 3


def axis_windows(L, w, s):
    """Origins of the windows along one axis: n = ceil((L - w) / s) + 1, o_i = min(i * s, L - w)."""
    assert 1 <= s <= w <= L
    n = -(-(L - w) // s) + 1
    return [min(i * s, L - w) for i in range(n)]


def axis_cover(L, w, s):
    """Per voxel of the axis, the list of the windows that cover it (every window tested)."""
    origins = axis_windows(L, w, s)
    return [[i for i, o in enumerate(origins) if o <= p < o + w] for p in range(L)]


def grid(shape, win, stride):
    """(per-axis origins, per-axis counts, Wn) for a (d, h, w) shape."""
    origins = [axis_windows(L, w, s) for L, w, s in zip(shape, triple(win), triple(stride))]
    counts = [len(o) for o in origins]
    return origins, counts, counts[0] * counts[1] * counts[2]


def window_box(index, shape, win, stride):
    """The (z, y, x) slices of window `index` (d-major numbering)."""
    origins, n, _ = grid(shape, win, stride)
    win = triple(win)
    a, rest = divmod(index, n[1] * n[2])
    b, c = divmod(rest, n[2])
    return tuple(slice(o[i], o[i] + w) for o, i, w in zip(origins, (a, b, c), win))


def occlude(x, fill, win, stride, first, count):
    """x: (c, d, h, w) float32, fill: c float32 -> (count, c, d, h, w): sample b has window min(first + b, Wn - 1) replaced by the
    channel's fill in every channel.  Bit patterns are copied (the work is done on a uint32 view)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    fill = np.asarray(fill, dtype=np.float32)
    _, _, wn = grid(x.shape[1:], win, stride)
    out = np.empty((count,) + x.shape, dtype=np.uint32)
    for b in range(count):
        out[b] = x.view(np.uint32)
        z, y, xx = window_box(min(first + b, wn - 1), x.shape[1:], win, stride)
        for ch in range(x.shape[0]):
            out[b, ch, z, y, xx] = fill[ch:ch + 1].view(np.uint32)[0]
    return out.view(np.float32)


def occlusion_map(base, scores, shape, win, stride):
    """base: k float32, scores: (Wn, k) float32 -> (k, d, h, w) float32: per class and voxel the fp64 sum of base - score over the covering
    windows in ascending (a, b, c) order, from 0.0, divided by their number in fp64 and rounded once."""
    base = np.asarray(base, dtype=np.float32).astype(np.float64)
    scores = np.asarray(scores, dtype=np.float32).astype(np.float64)
    _, n, wn = grid(shape, win, stride)
    assert scores.shape == (wn, base.shape[0])
    cover = [axis_cover(L, w, s) for L, w, s in zip(shape, triple(win), triple(stride))]
    delta = base[None, :] - scores                                            # (Wn, k), each difference rounded on its own
    out = np.empty((base.shape[0],) + tuple(shape), dtype=np.float32)
    for z in range(shape[0]):
        for y in range(shape[1]):
            for x in range(shape[2]):
                acc = np.zeros(base.shape[0], dtype=np.float64)
                count = 0
                for a in cover[0][z]:
                    for b in cover[1][y]:
                        for c in cover[2][x]:
                            acc = acc + delta[(a * n[1] + b) * n[2] + c]
                            count += 1
                out[:, z, y, x] = (acc / np.float64(count)).astype(np.float32)
    return out


def windows_meeting(cube, shape, win, stride):
    """Indices of the windows that share a voxel with `cube` (three slices)."""
    _, _, wn = grid(shape, win, stride)
    hit = []
    for i in range(wn):
        box = window_box(i, shape, win, stride)
        if all(max(b.start, c.start) < min(b.stop, c.stop) for b, c in zip(box, cube)):
            hit.append(i)
    return hit
