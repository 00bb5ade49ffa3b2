"""Geometry views as include/fenerf.h states them, on their numpy restatement (fenerf_amd/geometry_emulation.py -- the yardstick the GPU tests
hold fenerf_surface_points / fenerf_volume_sample_grad / fenerf_shade_normals to).  Nothing here touches the kernels."""
import os

import numpy as np
import pytest

from conftest import ROOT
from fenerf_amd import geometry_emulation as G, volume_emulation as V

F = np.float32
EPS = 2.0 ** -24          # unit roundoff of float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- surface points -----------------------------------------------------------------------------------------------------------------
def _rays(B, R, seed=0):
    rng = np.random.default_rng(seed)
    o = rng.normal(0, 1, (B, R, 3)).astype(F)
    d = rng.normal(0, 1, (B, R, 3)).astype(F)
    z = rng.uniform(0.5, 1.5, (B, R)).astype(F)
    a = rng.uniform(0.0, 1.0, (B, R)).astype(F)
    return o, d, z, a


@pytest.mark.parametrize("R", [1, 31, 32, 33])
def test_surface_points_against_fp64_and_pad_rows(R):
    B, amin = 2, 0.5
    o, d, z, a = _rays(B, R)
    Pp = G.padded_rows(R)
    assert Pp % 32 == 0 and Pp >= R and Pp - R < 32
    for alpha in (None, a):
        got = G.surface_points(o, d, z, alpha, amin)
        assert got.dtype == F and got.shape == (B, Pp, 3)
        z64 = z.astype(np.float64)
        if alpha is not None:
            z64 = np.where(a >= F(amin), z64 / a.astype(np.float64), z64)
        ref = o.astype(np.float64) + d.astype(np.float64) * z64[..., None]
        # three roundings (the quotient, the product, the sum) of values no larger than |o| + |d| z
        bound = 3 * EPS * (np.abs(o) + np.abs(d) * np.abs(z64[..., None])).max()
        assert np.abs(got[:, :R] - ref).max() <= bound
        for b in range(B):
            assert np.array_equal(_bits(got[b, R:]), _bits(np.repeat(got[b, R - 1:R], Pp - R, axis=0)))


def test_surface_points_alpha_threshold_and_non_finite_rows():
    amin = F(0.5)
    alpha = np.array([[np.nextafter(amin, F(0)), amin, np.nextafter(amin, F(1)), np.nan, 0.0, 1.0, 0.75, 0.75]], dtype=F)
    R = alpha.shape[1]
    o, d, z, _ = _rays(1, R, seed=1)
    z[0, 6] = np.inf          # a non-finite depth stays in its own row
    got = G.surface_points(o, d, z, alpha, amin)[0, :R]
    plain = (o[0] + (d[0] * z[0, :, None]).astype(F)).astype(F)
    divided = (o[0] + (d[0] * (z[0] / np.where(alpha[0] > 0, alpha[0], 1)).astype(F)[:, None]).astype(F)).astype(F)
    uses_alpha = np.array([False, True, True, False, False, True, True, True])
    for r in range(R):
        want = divided[r] if uses_alpha[r] else plain[r]
        if r == 6:
            assert not np.isfinite(got[r]).all()
        else:
            assert np.isfinite(got[r]).all() and np.array_equal(_bits(got[r]), _bits(want)), r
    assert not np.array_equal(plain[1], divided[1])          # the threshold matters for these rays


# ---- lattice gradient ---------------------------------------------------------------------------------------------------------------
ORIGIN, SPACING = (-4.0, 1.0, -0.5), (0.5, 0.25, 2.0)        # powers of two: lattice planes are hit exactly
SHAPES = [(3, 3, 3), (4, 4, 4), (5, 4, 7)]


def _lattice(shape, ld=3, seed=0):
    return np.random.default_rng(seed).uniform(-1, 1, tuple(shape) + (ld,)).astype(F)


def _sample_points(shape, seed=1):
    """random points in a box 1.5 cells larger than the lattice, every lattice node (all planes: t = 0, the shell faces t = 1 and t = n - 2,
    the last plane t = n - 1), mid-cell points, outside points and NaN / inf coordinates"""
    rng = np.random.default_rng(seed)
    o, s, n = np.array(ORIGIN, F), np.array(SPACING, F), np.array(shape)
    rand = (o + (rng.uniform(-1.5, 1.5 + (n - 1), (600, 3))).astype(F) * s).astype(F)
    idx = np.stack(np.meshgrid(*(np.arange(k) for k in shape), indexing="ij"), -1).reshape(-1, 3)
    nodes = (o + idx.astype(F) * s).astype(F)
    mids = (o + (idx.astype(F) + F(0.5)) * s).astype(F)
    on_plane = rand[:200].copy()          # one coordinate on a plane, the others free
    for j in range(len(on_plane)):
        k = j % 3
        on_plane[j, k] = o[k] + F(rng.integers(0, shape[k])) * s[k]
    special = []
    for k in range(3):
        for v in (np.nan, np.inf, -np.inf, F(o[k] - 3 * s[k]), F(o[k] + (shape[k] + 2) * s[k])):
            p = mids[len(mids) // 2].copy()
            p[k] = v
            special.append(p)
    return np.concatenate([rand, nodes, mids, on_plane, np.array(special, F)])


def _interior_by_definition(shape, pts):
    with np.errstate(all="ignore"):
        t = ((pts - np.array(ORIGIN, F)).astype(F) / np.array(SPACING, F)).astype(F)
        n = np.array(shape)
        inside = np.all((t >= 0) & (t <= (n - 1).astype(F)), axis=1)
        i = np.minimum(np.floor(np.where(np.isfinite(t), t, 0)).astype(np.int64), n - 2)
    return inside & np.all((i >= 1) & (i <= n - 3), axis=1), inside, i


@pytest.mark.parametrize("shape", SHAPES)
def test_lattice_gradient_interior_membership_and_zeros(shape):
    vol = _lattice(shape)
    pts = _sample_points(shape)
    want_interior, inside, i = _interior_by_definition(shape, pts)
    mask, ci, cf = G.interior(vol.shape, ORIGIN, SPACING, pts)
    assert np.array_equal(mask, want_interior)
    assert np.array_equal(ci, i[want_interior])
    if shape == (3, 3, 3):
        assert not mask.any()                                              # no interior cell at all
    else:
        assert mask.any() and (inside & ~mask).any() and (~inside).any()
    if shape == (4, 4, 4):
        assert (ci == 1).all()                                             # exactly one interior cell
    for ch in range(vol.shape[3]):
        g = G.volume_sample_grad(vol, ORIGIN, SPACING, pts, ch)
        assert g.dtype == F and g.shape == (len(pts), 3)
        assert np.array_equal(_bits(g[~mask]), np.zeros((int((~mask).sum()), 3), np.uint32))          # +0 everywhere else
        assert np.isfinite(g).all()
    if mask.any():
        assert (G.volume_sample_grad(vol, ORIGIN, SPACING, pts, 0)[mask] != 0).any()


@pytest.mark.parametrize("shape", SHAPES)
def test_cell_value_is_the_samplers_channel_bit_for_bit(shape):
    vol = _lattice(shape)
    pts = _sample_points(shape)
    n = tuple(shape)
    inside, i, f = V._cells(n, np.array(ORIGIN, F), np.array(SPACING, F), pts)
    rows = V.sample(vol, ORIGIN, SPACING, pts, -7.0)
    assert inside.sum() > 100
    for ch in range(vol.shape[3]):
        assert np.array_equal(_bits(G.cell_value(vol, ch, i, f)), _bits(rows[inside, ch]))


def test_lattice_gradient_of_an_affine_field():
    """sigma = a . x + b sampled at the lattice nodes (fp64, then rounded to float32): trilinear interpolation reproduces an affine field
    for ANY fractions, so V(i + e_k) - V(i - e_k) = 2 a_k spacing_k in exact arithmetic and the rounding of the fractions cancels.  What is
    left, to first order in eps = 2^-24 with M = max |sigma| over the lattice: a lattice value carries eps M; each of the three lerp levels
    adds at most 3 eps M (the rounding of 1 - f and of the two products changes the weights, which sum to one, by 2 eps; the sum rounds once);
    so a V carries 10 eps M, the difference of two 20 eps M plus its own rounding eps 2 M = 22 eps M, i.e. 11 eps M / spacing_k after the
    division by 2 spacing_k (the doubling is exact), whose own rounding adds eps |a_k| <= eps M / spacing_k: 12 eps M / spacing_k.  The factor
    (1 + 2^-10) covers the second-order terms.  Pins the sign, the axis order and the per-axis spacing: a = (3, -5, 7), three spacings."""
    shape = (6, 5, 7)
    origin, spacing = (0.37, -1.21, 2.5), (0.013, 0.11, 0.047)
    o, s = np.array(origin, F).astype(np.float64), np.array(spacing, F).astype(np.float64)
    a, b = np.array([3.0, -5.0, 7.0]), 0.75
    idx = np.stack(np.meshgrid(*(np.arange(k) for k in shape), indexing="ij"), -1)
    sigma = ((o + idx * s) @ a + b)
    vol = np.zeros(shape + (2,), F)
    vol[..., 1] = sigma.astype(F)
    M = float(np.abs(sigma).max())
    rng = np.random.default_rng(3)
    t = rng.uniform(1.0, np.array(shape) - 2.0, (4000, 3))
    pts = (o + t * s).astype(F)
    mask, _, _ = G.interior(vol.shape, origin, spacing, pts)
    assert mask.mean() > 0.95
    g = G.volume_sample_grad(vol, origin, spacing, pts, 1)[mask].astype(np.float64)
    for k in range(3):
        bound = 12 * EPS * M / s[k] * (1 + 2.0 ** -10)
        err = float(np.abs(g[:, k] - a[k]).max())
        print(f"affine field, axis {k}: max |g - a| {err:.3e}, bound {bound:.3e} (a_k = {a[k]}, spacing {s[k]:.4f})")
        assert err <= bound
        assert bound < 0.05 * abs(a[k])          # the bound separates a_k from every other candidate (sign, axis, spacing)
    assert np.array_equal(G.volume_sample_grad(vol, origin, spacing, pts, 0), np.zeros((len(pts), 3), F))


# ---- shading ------------------------------------------------------------------------------------------------------------------------
def test_shading_unit_normals_zero_gradient_and_back_faces():
    rng = np.random.default_rng(4)
    g = (rng.normal(0, 1, (2, 40, 3)) * 10.0 ** rng.uniform(-3, 3, (2, 40, 1))).astype(F)
    g[0, 0] = 0.0
    g[1, 1] = (0.0, 0.0, 5.0)          # n = (0, 0, -1): faces away from the light (0, 0, 1)
    g[1, 2] = (0.0, 0.0, -5.0)         # n = (0, 0, 1)
    normals, shaded = G.shade_normals(g, 40, None, None, (0.0, 0.0, 1.0), 0.25, 1.0, 0.5)
    assert normals.dtype == F and normals.shape == (2, 40, 3) and shaded.shape == (2, 40)
    length = np.linalg.norm(normals.astype(np.float64), axis=-1)
    nonzero = np.abs(g).max(-1) > 0
    assert np.abs(length[nonzero] - 1).max() <= 4 * EPS * 1.5          # sum of squares, sqrt, quotient: a few roundings
    assert np.array_equal(_bits(normals[0, 0]), np.zeros(3, np.uint32))          # zero gradient: (+0, +0, +0)
    assert shaded[0, 0] == F(0.25)
    # lam is exactly 0 for a back-facing normal: the shade is the ambient term, bit for bit
    assert np.array_equal(normals[1, 1], np.array([0, 0, -1], F)) and _bits(shaded[1, 1]) == _bits(F(0.25))
    assert np.array_equal(normals[1, 2], np.array([0, 0, 1], F)) and shaded[1, 2] == F(1.0)
    back = normals[..., 2] < 0
    assert back.any() and np.array_equal(_bits(shaded[back]), _bits(np.full(int(back.sum()), 0.25, F)))
    # the sign: the normal points against the gradient
    assert ((normals * g).sum(-1)[nonzero] < 0).all()
    # only the first R rows of an image are read
    n2, s2 = G.shade_normals(np.concatenate([g, np.full((2, 24, 3), np.nan, F)], axis=1), 40, None, None, (0.0, 0.0, 1.0), 0.25, 1.0, 0.5)
    assert np.array_equal(_bits(n2), _bits(normals)) and np.array_equal(_bits(s2), _bits(shaded))


def test_shading_camera_space_rotation_permutes_components():
    rng = np.random.default_rng(5)
    g = rng.normal(0, 1, (1, 16, 3)).astype(F)
    world, _ = G.shade_normals(g, 16, None, None)
    # cam2world = rotation by +90 degrees about y: its columns are the camera axes in world coordinates, x_cam = -z_world, z_cam = x_world
    c2w = np.array([[[0, 0, 1], [0, 1, 0], [-1, 0, 0]]], F)
    cam, shaded = G.shade_normals(g, 16, None, c2w, (0.0, 0.0, 1.0), 0.0, 1.0, 0.5)
    assert np.array_equal(cam[..., 0], -world[..., 2]) and np.array_equal(cam[..., 1], world[..., 1]) and np.array_equal(cam[..., 2], world[..., 0])
    assert np.array_equal(shaded, np.maximum(world[..., 0], 0))          # the light (0, 0, 1) is in camera space


def test_shading_invisible_rays_and_nan_rows():
    rng = np.random.default_rng(6)
    R = 12
    g = rng.normal(0, 1, (1, R, 3)).astype(F)
    g[0, 5, 1] = np.nan
    amin = F(0.5)
    alpha = rng.uniform(0.6, 1.0, (1, R)).astype(F)
    alpha[0, :5] = [0.0, np.nextafter(amin, F(0)), np.nan, amin, 1.5]
    normals, shaded = G.shade_normals(g, R, alpha, None, (0.0, 0.6, 0.8), 0.25, 0.5, amin)
    for r in (0, 1, 2):          # below the threshold, and NaN: zeros and the background
        assert np.array_equal(_bits(normals[0, r]), np.zeros(3, np.uint32)) and shaded[0, r] == F(0.5)
    assert np.abs(np.linalg.norm(normals[0, 3]) - 1) < 1e-6          # alpha == alpha_min is visible
    # alpha above 1 is clamped: the ray is opaque
    opaque, shade_opaque = G.shade_normals(g, R, None, None, (0.0, 0.6, 0.8), 0.25, 0.5, amin)
    assert _bits(shaded[0, 4]) == _bits(shade_opaque[0, 4])
    # a NaN gradient reaches the normal and the shade of its own ray only
    assert np.isnan(normals[0, 5]).all() and np.isnan(shaded[0, 5])
    others = np.arange(R) != 5
    assert np.isfinite(normals[0, others]).all() and np.isfinite(shaded[0, others]).all()
    clean = g.copy()
    clean[0, 5, 1] = 0.0
    n2, s2 = G.shade_normals(clean, R, alpha, None, (0.0, 0.6, 0.8), 0.25, 0.5, amin)
    assert np.array_equal(_bits(n2[0, others]), _bits(normals[0, others])) and np.array_equal(_bits(s2[0, others]), _bits(shaded[0, others]))
    # the blend: a * shade + (1 - a) * background
    r = 7
    lam = max(float(opaque[0, r] @ np.array([0.0, 0.6, 0.8])), 0.0)
    want = alpha[0, r] * (0.25 + 0.75 * lam) + (1 - alpha[0, r]) * 0.5
    assert abs(float(shaded[0, r]) - want) <= 8 * EPS


def test_geometry_entry_points_are_declared_exported_and_reachable():
    import sys
    from fenerf_amd import _lib, callers, native
    hdr = open(os.path.join(ROOT, "include", "fenerf.h")).read()
    l = _lib.lib()
    for name in ("fenerf_surface_points", "fenerf_volume_sample_grad", "fenerf_shade_normals"):
        assert name + "(" in hdr and name in _lib.EXPORTS and hasattr(l, name)
    assert "#define FENERF_ABI_VERSION 2" in hdr
    for f in (native.surface_points, native.volume_sample_grad, native.shade_normals, callers.render_geometry, callers.BakedField.render_geometry):
        assert callable(f)
    assert "torch" not in open(G.__file__).read()          # the yardstick is numpy alone
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import render_multiview
        import render_video_interpolation
    finally:
        sys.path.pop(0)
    for tool in (render_multiview, render_video_interpolation):
        opt = tool.build_parser().parse_args(["g.pth"])
        assert opt.geometry is False and render_multiview.geometry_options(opt) is False
        opt = tool.build_parser().parse_args(["g.pth", "--geometry", "--light", "1", "0", "1", "--ambient", "0.1"])
        assert render_multiview.geometry_options(opt) == dict(light=(1.0, 0.0, 1.0), ambient=0.1)
    assert render_multiview.build_parser().parse_args(["g.pth", "--geometry", "--baked", "64"]).baked == 64
