"""numpy restatement of fenerf_volume_sample (fenerf_amd/csrc/fenerf_volume.hip, include/fenerf.h "baked radiance lattice"): trilinear
rows of a channels-last lattice in the kernel's float32 arithmetic, operation by operation, so that the library's rows can be checked bit
for bit on the CPU side.

Conventions (include/fenerf.h states the same):
  - vol [n0][n1][n2][ld] float32; the first C of every ld floats are the channels; coordinate column k of a point belongs to lattice axis
    k; lattice point i_k lies at origin[k] + i_k * spacing[k].
  - t_k = (p_k - origin[k]) / spacing[k]; inside iff 0 <= t_k <= n_k - 1 on every axis (ordered: NaN / inf are outside).
  - inside: i_k = min(int(floor(t_k)), n_k - 2), f_k = t_k - i_k; every channel is three levels of a * (1 - f) + b * f, axis 2 first,
    then axis 1, then axis 0; every operation rounded to float32 on its own.
  - outside: zeros, with `outside_last` in channel C - 1."""
import numpy as np

F = np.float32


def ray_points(origins, dirs, z):
    """origins / dirs [..., 3], z [..., N] -> points [..., N, 3] = origins + dirs * z: one float32 multiply, one float32 add"""
    o, d, zz = (np.asarray(a, dtype=F) for a in (origins, dirs, z))
    return (o[..., None, :] + (d[..., None, :] * zz[..., None]).astype(F)).astype(F)


def _lerp(a, b, f):
    one_minus = (F(1.0) - f).astype(F)
    return ((a * one_minus).astype(F) + (b * f).astype(F)).astype(F)


def _cells(n, origin, spacing, pts):
    """steps 1-3 for pts [P,3]: -> (inside [P] bool, clamped cell index [Q,3] int64 and fractions [Q,3] float32 of the Q inside points)"""
    with np.errstate(all="ignore"):
        t = ((pts - origin[None, :]).astype(F) / spacing[None, :]).astype(F)
        hi = np.array([F(n[k] - 1) for k in range(3)], dtype=F)
        inside = np.all((t >= F(0.0)) & (t <= hi[None, :]), axis=1)
        ti = t[inside]
        i = np.minimum(np.floor(ti).astype(np.int64), np.array(n, dtype=np.int64)[None, :] - 2)
        f = (ti - i.astype(F)).astype(F)
    return inside, i, f


def sample(vol, origin, spacing, points, outside_last, C=None):
    """vol [n0,n1,n2,ld], origin / spacing [3], points [P,3] -> rows [P,C] float32 (C = ld unless given)"""
    vol = np.asarray(vol, dtype=F)
    n = vol.shape[:3]
    C = vol.shape[3] if C is None else int(C)
    assert vol.ndim == 4 and min(n) >= 2 and 1 <= C <= vol.shape[3]
    pts = np.asarray(points, dtype=F).reshape(-1, 3)
    o, s = np.asarray(origin, dtype=F), np.asarray(spacing, dtype=F)
    P = pts.shape[0]
    rows = np.zeros((P, C), dtype=F)
    rows[:, C - 1] = F(outside_last)
    with np.errstate(all="ignore"):
        inside, i, f = _cells(n, o, s, pts)
        i0, i1, i2 = i[:, 0], i[:, 1], i[:, 2]
        f0, f1, f2 = (f[:, k][:, None] for k in range(3))
        v = lambda d0, d1, d2: vol[i0 + d0, i1 + d1, i2 + d2, :C]
        c00, c01 = _lerp(v(0, 0, 0), v(0, 0, 1), f2), _lerp(v(0, 1, 0), v(0, 1, 1), f2)
        c10, c11 = _lerp(v(1, 0, 0), v(1, 0, 1), f2), _lerp(v(1, 1, 0), v(1, 1, 1), f2)
        c0, c1 = _lerp(c00, c01, f1), _lerp(c10, c11, f1)
        rows[inside] = _lerp(c0, c1, f0)
    return rows
