"""numpy restatement of the geometry-view kernels (fenerf_amd/csrc/fenerf_geometry.hip, include/fenerf.h "geometry views"):
fenerf_surface_points, fenerf_volume_sample_grad and fenerf_shade_normals in the kernels' float32 arithmetic, operation by operation, so that
the library's outputs can be checked bit for bit on the CPU side.  The lattice part reuses volume_emulation's cell arithmetic and lerp.

Conventions (include/fenerf.h states the same):
  - surface point: z = depth, or depth / alpha where alpha is given and alpha >= alpha_min (ordered: NaN is false); p = origin + dir * z,
    one multiply then one add; rows R .. Pp - 1 of an image (Pp = R rounded up to a multiple of 32) repeat the point of its ray R - 1.
  - lattice gradient: a point is interior iff it is inside and 1 <= i_k <= n_k - 3 on every axis; there
    g_k = (V(i + e_k) - V(i - e_k)) / (spacing[k] + spacing[k]) with V(j) = the sampler's trilinear value at cell j with the POINT's
    fractions; elsewhere (0, 0, 0).
  - shading: n = -g / |g| (zeros for |g| = 0), optionally m = R^T n, Lambert with an ambient term, alpha-blended onto `background`;
    a ray with alpha < alpha_min (or NaN) gets a zero normal and `background`."""
import numpy as np

from .volume_emulation import F, _cells, _lerp


def padded_rows(R):
    """rows per image of the surface points: R rounded up to a multiple of 32"""
    return (int(R) + 31) // 32 * 32


def surface_points(origins, dirs, depth, alpha=None, alpha_min=0.5):
    """origins / dirs [B,R,3], depth / alpha [B,R] -> points [B,Pp,3] float32"""
    o, d, z = (np.asarray(a, dtype=F) for a in (origins, dirs, depth))
    B, R = z.shape
    with np.errstate(all="ignore"):
        if alpha is not None:
            a = np.asarray(alpha, dtype=F)
            assert np.isfinite(alpha_min) and alpha_min > 0
            use = a >= F(alpha_min)
            z = np.where(use, (z / np.where(use, a, F(1.0))).astype(F), z)
        p = (o + (d * z[..., None]).astype(F)).astype(F)
    Pp = padded_rows(R)
    if R == 0:
        return np.zeros((B, 0, 3), dtype=F)
    return np.concatenate([p, np.repeat(p[:, -1:], Pp - R, axis=1)], axis=1)


def cell_value(vol, channel, i, f):
    """V(i): the sampler's step-4 value of `channel` at cells i [Q,3] (int) with fractions f [Q,3]: seven lerps, axis 2, axis 1, axis 0"""
    i0, i1, i2 = i[:, 0], i[:, 1], i[:, 2]
    f0, f1, f2 = f[:, 0], f[:, 1], f[:, 2]
    v = lambda d0, d1, d2: vol[i0 + d0, i1 + d1, i2 + d2, channel]
    with np.errstate(all="ignore"):
        c00, c01 = _lerp(v(0, 0, 0), v(0, 0, 1), f2), _lerp(v(0, 1, 0), v(0, 1, 1), f2)
        c10, c11 = _lerp(v(1, 0, 0), v(1, 0, 1), f2), _lerp(v(1, 1, 0), v(1, 1, 1), f2)
        c0, c1 = _lerp(c00, c01, f1), _lerp(c10, c11, f1)
        return _lerp(c0, c1, f0)


def interior(shape, origin, spacing, points):
    """-> (interior [P] bool, cell index [Q,3] and fractions [Q,3] of the Q interior points)"""
    n = np.array(shape[:3], dtype=np.int64)
    pts = np.asarray(points, dtype=F).reshape(-1, 3)
    inside, i, f = _cells(tuple(int(k) for k in n), np.asarray(origin, dtype=F), np.asarray(spacing, dtype=F), pts)
    keep = np.all((i >= 1) & (i <= n[None, :] - 3), axis=1)
    mask = np.zeros(pts.shape[0], dtype=bool)
    mask[np.flatnonzero(inside)[keep]] = True
    return mask, i[keep], f[keep]


def volume_sample_grad(vol, origin, spacing, points, channel):
    """vol [n0,n1,n2,ld], points [P,3] -> grads [P,3] float32"""
    vol = np.asarray(vol, dtype=F)
    assert vol.ndim == 4 and min(vol.shape[:3]) >= 2 and 0 <= channel < vol.shape[3]
    s = np.asarray(spacing, dtype=F)
    mask, i, f = interior(vol.shape, origin, spacing, points)
    g = np.zeros((mask.shape[0], 3), dtype=F)
    with np.errstate(all="ignore"):
        for k in range(3):
            e = np.zeros((1, 3), dtype=np.int64)
            e[0, k] = 1
            diff = (cell_value(vol, channel, i + e, f) - cell_value(vol, channel, i - e, f)).astype(F)
            g[mask, k] = (diff / (s[k] + s[k]).astype(F)).astype(F)
    return g


def shade_normals(grads, R, alpha=None, cam2world=None, light=(0.0, 0.0, 1.0), ambient=0.25, background=1.0, alpha_min=0.5):
    """grads [B,rows,3] (rows >= R; the first R rows of an image are read), alpha [B,R] or None, cam2world [B,3,3] or None
    -> (normals [B,R,3], shaded [B,R]) float32"""
    g = np.asarray(grads, dtype=F)[:, :R]
    l = np.asarray(light, dtype=F)
    amb, bg = F(ambient), F(background)
    with np.errstate(all="ignore"):
        gx, gy, gz = g[..., 0], g[..., 1], g[..., 2]
        s = (((gx * gx).astype(F) + (gy * gy).astype(F)).astype(F) + (gz * gz).astype(F)).astype(F)
        length = np.sqrt(s).astype(F)
        zero = length == F(0.0)
        safe = np.where(zero, F(1.0), length)
        n = np.where(zero[..., None], F(0.0), ((-g) / safe[..., None]).astype(F)).astype(F)
        if cam2world is not None:
            Rm = np.asarray(cam2world, dtype=F)[:, None]          # [B,1,3,3]
            m = np.stack([(((Rm[..., 0, j] * n[..., 0]).astype(F) + (Rm[..., 1, j] * n[..., 1]).astype(F)).astype(F)
                           + (Rm[..., 2, j] * n[..., 2]).astype(F)).astype(F) for j in range(3)], axis=-1)
        else:
            m = n
        if alpha is None:
            a = np.ones(s.shape, dtype=F)
            visible = np.ones(s.shape, dtype=bool)
        else:
            raw = np.asarray(alpha, dtype=F)
            a = np.where(raw < F(0.0), F(0.0), raw)
            a = np.where(a > F(1.0), F(1.0), a).astype(F)
            visible = raw >= F(alpha_min)
        d = (((m[..., 0] * l[0]).astype(F) + (m[..., 1] * l[1]).astype(F)).astype(F) + (m[..., 2] * l[2]).astype(F)).astype(F)
        lam = np.where(d < F(0.0), F(0.0), d).astype(F)
        shade = (amb + ((F(1.0) - amb).astype(F) * lam).astype(F)).astype(F)
        blended = ((a * shade).astype(F) + ((F(1.0) - a).astype(F) * bg).astype(F)).astype(F)
        normals = np.where(visible[..., None], m, F(0.0)).astype(F)
        shaded = np.where(visible, blended, bg).astype(F)
    return normals, shaded
