"""numpy restatement of the surface mesh behind the mesh-based shape features (`mmnn_radiomics_mesh`, csrc/radiomics_mesh.hip).

The contract (include/mmnn_sts.h), restated.  The ROI (bin != 0) is padded with one layer of empty voxels on every side; a
cell is a 2 x 2 x 2 block of corners with origin o in -1 .. extent - 1 per axis; corner k of a cell is o + (k & 1, k >> 1 & 1, k >> 2 & 1)
in (x, y, z), bit k of its configuration says whether that corner is in the ROI.  Coordinates are doubled voxel indices, so the midpoint
of every cell edge is an integer triple.

    vertices     every cell edge whose corners differ carries one vertex at its midpoint
    segments     on each of the six faces the four corners are visited counter-clockwise as seen from outside the cell; every maximal
                 run of set corners is cut off by one directed segment from the crossing where the run starts to the one where it ends
    loops        every vertex ends one segment and starts another: following them gives disjoint closed loops
    triangles    a loop is rotated to start at its lowest-numbered edge v0 and cut into the fan (v0, v_i, v_i+1); the loops of a cell are
                 taken in the order of their lowest edge.  Edge 4 a + p + 2 q runs along axis a (x 0, y 1, z 2) at the position (p, q)
                 of the two other axes, ascending
    orientation  as directed above the normals (b - a) x (c - a) point out of the ROI: the signed volume of a solid is positive

This file derives the table from COORDINATES: it sorts a face's corners by their angle around the outward normal and follows points.
tools/gen_mesh_table.py, which writes the header the library is built with, works on edge numbers and face tables instead; the two share
no code, and tests/test_radiomics_mesh_cpu.py holds the library's table against this one.

What the device returns, restated: `restate(roi, L)`.
    cfg[256]     cells per configuration, all (x + 1)(y + 1)(z + 1) cells counted
    n_vertices, n_triangles, volume48 = sum over triangles of a . (b x c)
    area         sum_c cfg[c] A_c in index order, A_c = sum over the configuration's triangles of |cof(L) n| / 8, n the integer normal
    q[4]         the largest q = ((dt0)^2 + (dt1)^2) + (dt2)^2 over all unordered vertex pairs, self-pairs included, with
                 t_r = (L[r][0] vx + L[r][1] vy) + L[r][2] vz, and over the pairs whose z, y, x coordinate agrees (Slice, Column, Row)
"""
import math

import numpy as np

MESH_SHAPE = ("MeshVolume", "SurfaceArea", "SurfaceVolumeRatio", "Sphericity", "Maximum3DDiameter", "Maximum2DDiameterSlice",
              "Maximum2DDiameterColumn", "Maximum2DDiameterRow")
INTEGERS = ("n_vertices", "n_triangles", "volume48")
DIAMETERS = ("q3d", "q_slice", "q_column", "q_row")
_TABLE = None


def _edge_number(p):
    """The number of the cell edge whose midpoint is the doubled local point p (exactly one odd coordinate)."""
    a = [k for k in range(3) if p[k] == 1]
    assert len(a) == 1 and all(v in (0, 1, 2) for v in p)
    u, w = [k for k in range(3) if k != a[0]]
    return 4 * a[0] + p[u] // 2 + 2 * (p[w] // 2)


def _cell_triangles(cfg):
    """The triangles of one configuration as triples of doubled local points, from the rule."""
    inside = lambda c: bool(cfg >> (c[0] + 2 * c[1] + 4 * c[2]) & 1)
    follow = {}
    for axis in range(3):
        for side in (0, 1):
            normal = np.zeros(3)
            normal[axis] = 1.0 if side else -1.0
            u = np.zeros(3)
            u[(axis + 1) % 3] = 1.0
            w = np.cross(normal, u)                                     # (u, w, normal) right-handed: angles grow counter-clockwise from outside
            corners = [c for c in np.ndindex(2, 2, 2) if c[axis] == side]
            centre = np.mean(corners, axis=0)
            corners.sort(key=lambda c: math.atan2(np.dot(c - centre, w), np.dot(c - centre, u)))
            flags = [inside(c) for c in corners]
            if all(flags) or not any(flags):
                continue
            for k in range(4):
                if not flags[k] or flags[k - 1]:
                    continue
                end = k                                                 # a run of set corners starts at k
                while flags[(end + 1) % 4]:
                    end += 1
                start_pt = tuple(int(a + b) for a, b in zip(corners[k - 1], corners[k]))
                end_pt = tuple(int(a + b) for a, b in zip(corners[end % 4], corners[(end + 1) % 4]))
                assert start_pt not in follow
                follow[start_pt] = end_pt
    assert set(follow) == set(follow.values())                          # every vertex ends one segment and starts another
    loops, seen = [], set()
    for p in sorted(follow, key=_edge_number):
        if p in seen:
            continue
        loop = [p]
        seen.add(p)
        while follow[loop[-1]] != p:
            loop.append(follow[loop[-1]])
            seen.add(loop[-1])
        loops.append(loop)                                              # starts at its lowest edge; the loops in the order of that edge
    return [(lp[0], lp[i], lp[i + 1]) for lp in loops for i in range(1, len(lp) - 1)]


def table():
    """(tri [256][16] int8: edge numbers, -1 behind the last, the count in [15]; points: per configuration the (T, 3, 3) local points)."""
    global _TABLE
    if _TABLE is None:
        tri, pts = np.full((256, 16), -1, dtype=np.int8), []
        for cfg in range(256):
            t = _cell_triangles(cfg)
            assert len(t) <= 5
            tri[cfg, :3 * len(t)] = [_edge_number(p) for f in t for p in f]
            tri[cfg, 15] = len(t)
            pts.append(np.array(t, dtype=np.int64).reshape(len(t), 3, 3))
        _TABLE = (tri, pts)
    return _TABLE


def shortcut_tables():
    """(L48 [256], N [256][3]): sum of a . (b x c) and of (b - a) x (c - a) over a configuration's triangles, local doubled coordinates."""
    l48, nsum = np.zeros(256, dtype=np.int64), np.zeros((256, 3), dtype=np.int64)
    for cfg, t in enumerate(table()[1]):
        if len(t):
            l48[cfg] = np.einsum("ti,ti->", t[:, 0], np.cross(t[:, 1], t[:, 2]))
            nsum[cfg] = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]).sum(axis=0)
    return l48, nsum


def configurations(roi):
    """The configuration byte of every cell: (x + 1, y + 1, z + 1) uint8, index = origin + 1."""
    p = np.pad(np.asarray(roi, dtype=bool), 1)
    x, y, z = p.shape
    cfg = np.zeros((x - 1, y - 1, z - 1), dtype=np.int64)
    for k in range(8):
        dx, dy, dz = k & 1, k >> 1 & 1, k >> 2 & 1
        cfg |= p[dx:x - 1 + dx, dy:y - 1 + dy, dz:z - 1 + dz].astype(np.int64) << k
    return cfg


def triangles(roi):
    """Every triangle of the mesh, (T, 3, 3) int64 doubled coordinates (voxel i sits at 2 i)."""
    cfg, pts = configurations(roi), table()[1]
    out = []
    for c in np.unique(cfg):
        if len(pts[c]):
            origins = 2 * (np.argwhere(cfg == c).astype(np.int64) - 1)
            out.append((origins[:, None, None, :] + pts[c][None]).reshape(-1, 3, 3))
    return np.concatenate(out) if out else np.zeros((0, 3, 3), dtype=np.int64)


def vertices(roi):
    """The vertices, from the lattice edges alone (no table): (V, 3) int64 doubled coordinates, sorted."""
    p = np.pad(np.asarray(roi, dtype=bool), 1)
    out = []
    for axis in range(3):
        a, b = np.moveaxis(p, axis, 0)[:-1], np.moveaxis(p, axis, 0)[1:]
        at = np.argwhere(np.moveaxis(a != b, 0, axis)).astype(np.int64)      # the lower corner, padded index
        v = 2 * (at - 1)
        v[:, axis] += 1
        out.append(v)
    v = np.concatenate(out)
    return v[np.lexsort((v[:, 0], v[:, 1], v[:, 2]))]


def balanced(tris):
    """Every directed edge occurs as often as its reverse (closed; an undirected edge may be used more than twice)."""
    if not len(tris):
        return True
    e = np.concatenate([np.concatenate([tris[:, k], tris[:, (k + 1) % 3]], axis=1) for k in range(3)])
    fwd, nf = np.unique(e, axis=0, return_counts=True)
    rev, nr = np.unique(e[:, [3, 4, 5, 0, 1, 2]], axis=0, return_counts=True)
    return np.array_equal(fwd, rev) and np.array_equal(nf, nr)


def volume48(tris):
    return int(np.einsum("ti,ti->t", tris[:, 0], np.cross(tris[:, 1], tris[:, 2])).sum()) if len(tris) else 0


def cofactor(L):
    """cof(L): row r is the cross product of the two other rows of L, so that (L a) x (L b) = cof(L) (a x b)."""
    L = np.asarray(L, dtype=np.float64).reshape(3, 3)
    return np.array([[L[(r + 1) % 3][(c + 1) % 3] * L[(r + 2) % 3][(c + 2) % 3] - L[(r + 1) % 3][(c + 2) % 3] * L[(r + 2) % 3][(c + 1) % 3]
                      for c in range(3)] for r in range(3)], dtype=np.float64)


def _triangle_area(C, n):
    w = [(C[r][0] * np.float64(n[0]) + C[r][1] * np.float64(n[1])) + C[r][2] * np.float64(n[2]) for r in range(3)]
    return np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]) * 0.125


def cell_areas(L):
    """A_c [256]: the area, in the units of L, of each configuration's triangles, summed in table order."""
    C, out = cofactor(L), np.zeros(256, dtype=np.float64)
    for cfg, t in enumerate(table()[1]):
        s = np.float64(0.0)
        for a, b, c in t:
            s = s + _triangle_area(C, np.cross(b - a, c - a))
        out[cfg] = s
    return out


def area(hist, L):
    """(sum_c cfg[c] A_c in index order, sum of the terms' magnitudes)."""
    A, s = cell_areas(L), np.float64(0.0)
    for c in range(256):
        s = s + np.float64(int(hist[c])) * A[c]
    return float(s), float(s)                                            # every term is non-negative: the scale is the sum itself


def exact_area(hist, L, digits=40):
    """The same sum in mpmath from the integer normals and the doubles of L."""
    import mpmath
    with mpmath.workdps(digits):
        Lm = [[mpmath.mpf(float(v)) for v in row] for row in np.asarray(L, dtype=np.float64).reshape(3, 3)]
        C = [[Lm[(r + 1) % 3][(c + 1) % 3] * Lm[(r + 2) % 3][(c + 2) % 3] - Lm[(r + 1) % 3][(c + 2) % 3] * Lm[(r + 2) % 3][(c + 1) % 3]
              for c in range(3)] for r in range(3)]
        total = mpmath.mpf(0)
        for cfg, t in enumerate(table()[1]):
            if not hist[cfg]:
                continue
            for a, b, c in t:
                n = [int(v) for v in np.cross(b - a, c - a)]
                w = [C[r][0] * n[0] + C[r][1] * n[1] + C[r][2] * n[2] for r in range(3)]
                total += int(hist[cfg]) * mpmath.sqrt(w[0] ** 2 + w[1] ** 2 + w[2] ** 2) / 8
        return total


def area_deviation(value, hist, L):
    """|value - exact| relative to the sum of the terms' magnitudes (the exact sum: every term is non-negative)."""
    import mpmath
    ex = exact_area(hist, L)
    with mpmath.workdps(40):
        return float(abs(mpmath.mpf(float(value)) - ex) / ex) if ex != 0 else abs(float(value))


def squared_diameters(v, L, chunk=512):
    """The four largest q over all unordered vertex pairs (self-pairs included: 0 at least), bit for bit as the device computes them."""
    L = np.asarray(L, dtype=np.float64).reshape(3, 3)
    vd = v.astype(np.float64)
    t = np.stack([(L[r][0] * vd[:, 0] + L[r][1] * vd[:, 1]) + L[r][2] * vd[:, 2] for r in range(3)], axis=1)
    best = np.zeros(4, dtype=np.float64)
    for i0 in range(0, len(v), chunk):
        d = t[i0:i0 + chunk, None, :] - t[None, :, :]
        q = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        best[0] = max(best[0], q.max())
        for k, ax in ((1, 2), (2, 1), (3, 0)):                           # Slice: z agrees, Column: y, Row: x
            same = v[i0:i0 + chunk, None, ax] == v[None, :, ax]
            best[k] = max(best[k], np.where(same, q, 0.0).max())
    return best


def restate(roi, L=None, flagged=False):
    """What `mmnn_radiomics_mesh` returns for the ROI `roi` (x, y, z bool) and the linear part L."""
    L = np.eye(3) if L is None else np.asarray(L, dtype=np.float64).reshape(3, 3)
    nan = float("nan")
    if flagged:
        return {"cfg": np.zeros(256, dtype=np.int64), "n_vertices": 0, "n_triangles": 0, "volume48": 0, "area": nan, "area_scale": nan,
                "q": np.full(4, nan), "flagged": True, "L": L}
    hist = np.bincount(configurations(roi).ravel(), minlength=256).astype(np.int64)
    tris, v = triangles(roi), vertices(roi)
    A, scale = area(hist, L)
    return {"cfg": hist, "n_vertices": len(v), "n_triangles": len(tris), "volume48": volume48(tris), "area": A, "area_scale": scale,
            "q": squared_diameters(v, L), "flagged": False, "L": L, "vertices": v, "triangles": tris}


def derived(volume48_, area_, q, L):
    """The eight columns from the device's outputs, as `radiomics.mesh_features` must compute them."""
    det = abs(float(np.linalg.det(np.asarray(L, dtype=np.float64).reshape(3, 3))))
    V = volume48_ / 48.0 * det
    out = {"MeshVolume": V, "SurfaceArea": area_, "SurfaceVolumeRatio": area_ / V, "Sphericity": (36.0 * math.pi * V * V) ** (1.0 / 3.0) / area_}
    for name, s in zip(MESH_SHAPE[4:], q):
        out[name] = math.sqrt(s) / 2.0
    return out
