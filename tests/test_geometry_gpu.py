"""fenerf_surface_points / fenerf_volume_sample_grad / fenerf_shade_normals (fenerf_amd/csrc/fenerf_geometry.hip) against their numpy
restatement (fenerf_amd/geometry_emulation.py, itself held to its definitions by tests/test_geometry_cpu.py) bit for bit, their refusals, and
callers.render_geometry end to end on the exact and the baked route.  "Bit for bit" treats every NaN as the same value: which NaN an
operation returns is not part of the contract."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
from test_gpu_parity import DEV, N_, T, load_golden, proc
from test_mesh_gpu import GRID, _generator
from test_geometry_cpu import ORIGIN, SPACING, _lattice, _sample_points
from fenerf_amd import _lib, callers, geometry_emulation as E, native
from fenerf_amd.generators import volumetric_rendering as VR

pytestmark = pytest.mark.gpu

F = np.float32


def _same(got, want):
    """equal bits, or both NaN"""
    got, want = np.ascontiguousarray(got, dtype=F), np.ascontiguousarray(want, dtype=F)
    assert got.shape == want.shape, (got.shape, want.shape)
    differ = (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))
    if differ.any():
        where = np.argwhere(differ)
        print(f"{int(differ.sum())} of {differ.size} values differ; the first at {tuple(where[0])}: got {got[tuple(where[0])]!r}, want {want[tuple(where[0])]!r}; "
              f"indices {[tuple(w) for w in where[:8]]}")
    return not differ.any()


# ---- 1. surface points --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 31, 32, 33, 100])
def test_surface_points_vs_emulation_bit_for_bit(R):
    B, amin = 2, F(0.5)
    rng = np.random.default_rng(R)
    o = rng.normal(0, 1, (B, R, 3)).astype(F)
    d = rng.normal(0, 1, (B, R, 3)).astype(F)
    z = rng.uniform(0.5, 1.5, (B, R)).astype(F)
    a = rng.uniform(0.0, 1.0, (B, R)).astype(F)
    special = [np.nextafter(amin, F(0)), amin, np.nextafter(amin, F(1)), np.nan, 0.0, np.inf]
    for j, v in enumerate(special):          # image 1: alpha below, at and above alpha_min, NaN, 0, inf (as far as R reaches)
        if j < R:
            a[1, j] = v
    if R > 8:
        z[0, 7], z[0, 8], o[1, R - 1, 1] = np.inf, np.nan, np.nan          # a non-finite depth; a NaN origin in the row the pad rows repeat
    for alpha in (None, a):
        got = native.surface_points(T(o), T(d), T(z), None if alpha is None else T(alpha), float(amin))
        Pp = E.padded_rows(R)
        assert got.shape == (B, Pp, 3) and got.dtype == torch.float32 and got.is_cuda
        want = E.surface_points(o, d, z, alpha, amin)
        assert _same(N_(got), want), (R, alpha is None)
        if R > 8:
            finite_rows = np.isfinite(want[0, :R]).all(-1)
            assert finite_rows.sum() == R - 2 and not finite_rows[7] and not finite_rows[8]          # non-finite inputs stay in their own rows


# ---- 2. lattice gradient ------------------------------------------------------------------------------------------------------------
def _device_lattice(vol, offset):
    if not offset:
        return T(vol)
    flat = torch.empty(vol.size + 1, dtype=torch.float32, device=DEV)          # the same lattice one float off its allocation's base
    off = flat[1:].view(*vol.shape)
    off.copy_(T(vol))
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    return off


@pytest.mark.parametrize("ld", [24, 23])
@pytest.mark.parametrize("shape", [(4, 4, 4), (5, 4, 7), (9, 6, 33)])
def test_volume_sample_grad_vs_emulation_bit_for_bit(shape, ld):
    C_ = 22
    vol = _lattice(shape, ld, seed=2)
    pool = _sample_points(shape, seed=3)          # a box 1.5 cells larger than the lattice, nodes (every plane, both shell faces), outside, NaN / inf
    pool = pool[np.random.default_rng(4).permutation(len(pool))]
    assert len(pool) >= 257
    for offset in (False, True):
        dvol = _device_lattice(vol, offset)
        for ch in (0, 9, C_ - 1):
            want_all = E.volume_sample_grad(vol, ORIGIN, SPACING, pool, ch)
            for P in (0, 1, 63, 64, 65, 257, len(pool)):
                got = native.volume_sample_grad(dvol, ORIGIN, SPACING, T(pool[:P].reshape(P, 3)), ch)
                assert got.shape == (P, 3) and got.dtype == torch.float32 and got.is_cuda
                assert _same(N_(got), want_all[:P]), (shape, ld, offset, ch, P)
    mask, _, _ = E.interior(vol.shape, ORIGIN, SPACING, pool)
    assert mask.any() and (~mask).any() and np.isfinite(want_all).all() and (want_all[mask] != 0).any()
    # a lattice with an Inf and a NaN entry: they reach the rows that read them, nothing else
    bad = vol.copy()
    bad[1, 1, 1, C_ - 1], bad[shape[0] - 2, 2, shape[2] - 2, C_ - 1] = np.inf, np.nan
    got = N_(native.volume_sample_grad(T(bad), ORIGIN, SPACING, T(pool), C_ - 1))
    want = E.volume_sample_grad(bad, ORIGIN, SPACING, pool, C_ - 1)
    assert _same(got, want)
    assert (~np.isfinite(want)).any() and np.array_equal(np.isfinite(want).all(-1) | mask, np.ones(len(pool), bool))
    untouched = np.isfinite(want).all(-1)
    assert _same(got[untouched], want_all[untouched])


# ---- 3. shading ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 63, 64, 65])
def test_shade_normals_vs_emulation_bit_for_bit(R):
    B, amin = 2, 0.5
    rng = np.random.default_rng(10 + R)
    c2w = np.stack([np.linalg.qr(rng.normal(size=(3, 3)))[0] for _ in range(B)]).astype(F)
    light = (0.26726124, -0.53452248, 0.80178373)
    for rows in (R, R + 31):
        g = (rng.normal(0, 1, (B, rows, 3)) * 10.0 ** rng.uniform(-3, 3, (B, rows, 1))).astype(F)
        a = rng.uniform(-0.1, 1.1, (B, R)).astype(F)
        g[0, 0] = 0.0
        if R > 8:
            g[0, 1, 2], g[0, 2, 0], g[1, 3], g[1, 4, 1] = np.nan, np.inf, (-0.0, 0.0, -0.0), -np.inf
            a[0, 5], a[1, 6], a[0, 7], a[0, 1] = np.nan, 0.5, np.nextafter(F(0.5), F(0)), 0.9          # ray (0, 1): visible, NaN gradient
        for alpha in (None, a):
            for cam in (None, c2w):
                normals, shaded = native.shade_normals(T(g), R, None if alpha is None else T(alpha), None if cam is None else T(cam), light, 0.25, 0.9, amin)
                wn, ws = E.shade_normals(g, R, alpha, cam, light, 0.25, 0.9, amin)
                assert normals.shape == (B, R, 3) and shaded.shape == (B, R)
                assert _same(N_(normals), wn) and _same(N_(shaded), ws), (R, rows, alpha is None, cam is None)
                only_n, none = native.shade_normals(T(g), R, None if alpha is None else T(alpha), None if cam is None else T(cam), light, 0.25, 0.9, amin,
                                                    want_shaded=False)
                assert none is None and _same(N_(only_n), wn)
        if R > 8:
            assert np.isnan(wn[0, 1]).all() and np.isnan(ws[0, 1]) and np.isfinite(wn[0, 8:]).all() and np.isfinite(ws[0, 8:]).all()


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------------
PATTERN = 1234.5


def _refused(fn, good, faults, outputs):
    l = _lib.lib()
    for change, text in faults:
        rc = fn(*dict(good, **change).values())
        msg = l.fenerf_last_error().decode()
        assert rc == _lib.E_INVALID and msg and text in msg, (fn.__name__, change, rc, msg)
    torch.cuda.synchronize()
    for t in outputs:
        assert bool((t == PATTERN).all()), fn.__name__          # nothing was launched


def test_c_abi_refusals():
    l = _lib.lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    f3 = lambda *v: (C.c_float * 3)(*v)
    nan, inf = float("nan"), float("inf")
    full = lambda *shape: torch.full(shape, PATTERN, dtype=torch.float32, device=DEV)
    B, R = 2, 5
    rays, scal = torch.zeros((B * R, 3), device=DEV), torch.ones((B * R,), device=DEV)
    # fenerf_surface_points
    points = full(B, 32, 3)
    good = dict(B=B, R=R, origins=p(rays), dirs=p(rays), depth=p(scal), alpha=p(scal), alpha_min=0.5, points=p(points), stream=None)
    _refused(l.fenerf_surface_points, good,
             [(dict(origins=None), "NULL"), (dict(dirs=None), "NULL"), (dict(depth=None), "NULL"), (dict(points=None), "NULL"), (dict(B=-1), "negative count"),
              (dict(R=-1), "negative count"), (dict(alpha_min=0.0), "alpha_min"), (dict(alpha_min=-0.5), "alpha_min"), (dict(alpha_min=nan), "alpha_min"),
              (dict(alpha_min=inf), "alpha_min")], [points])
    assert l.fenerf_surface_points(*dict(good, B=0).values()) == _lib.OK and l.fenerf_surface_points(*dict(good, R=0).values()) == _lib.OK
    assert l.fenerf_surface_points(*dict(good, alpha=None, alpha_min=nan).values()) == _lib.OK          # alpha_min is not read without alpha
    torch.cuda.synchronize()
    assert not bool((points[:, :R] == PATTERN).any())
    # fenerf_volume_sample_grad
    vol = torch.zeros((4, 4, 4, 24), device=DEV)
    P = 7
    pts, grads = torch.zeros((P, 3), device=DEV), full(P, 3)
    good = dict(vol=p(vol), n0=4, n1=4, n2=4, ld=24, channel=21, origin=f3(0, 0, 0), spacing=f3(0.1, 0.1, 0.1), P=P, points=p(pts), grads=p(grads), stream=None)
    _refused(l.fenerf_volume_sample_grad, good,
             [(dict(vol=None), "NULL"), (dict(origin=None), "NULL"), (dict(spacing=None), "NULL"), (dict(points=None), "NULL"), (dict(grads=None), "NULL"),
              (dict(n0=1), "at least 2 points"), (dict(n1=1), "at least 2 points"), (dict(n2=0), "at least 2 points"),
              (dict(n0=2048, n1=2048, n2=512), "lattice points"), (dict(channel=-1), "channel"), (dict(channel=24), "channel"),
              (dict(spacing=f3(0.0, 0.1, 0.1)), "finite and positive"), (dict(spacing=f3(0.1, -0.1, 0.1)), "finite and positive"),
              (dict(spacing=f3(0.1, 0.1, inf)), "finite and positive"), (dict(spacing=f3(nan, 0.1, 0.1)), "finite and positive"), (dict(P=-1), "negative count")],
             [grads])
    assert l.fenerf_volume_sample_grad(*dict(good, P=0).values()) == _lib.OK
    small = torch.zeros((3, 2, 3, 24), device=DEV)          # an axis with fewer than 4 points: valid, every row zero
    assert l.fenerf_volume_sample_grad(*dict(good, vol=p(small), n0=3, n1=2, n2=3).values()) == _lib.OK
    torch.cuda.synchronize()
    assert bool((grads == 0).all())
    # fenerf_shade_normals
    g, normals, shaded = torch.ones((B, 8, 3), device=DEV), full(B * R, 3), full(B * R)
    good = dict(B=B, R=R, rows_per_image=8, grads=p(g), alpha=p(scal), cam2world=None, light=f3(0, 0, 1), ambient=0.25, background=1.0, alpha_min=0.5,
                normals=p(normals), shaded=p(shaded), stream=None)
    _refused(l.fenerf_shade_normals, good,
             [(dict(grads=None), "NULL"), (dict(normals=None), "NULL"), (dict(light=None), "NULL"), (dict(rows_per_image=4), "rows_per_image < R"),
              (dict(B=-1), "negative count"), (dict(R=-1), "negative count"), (dict(rows_per_image=-1, R=-2), "negative count"),
              (dict(ambient=nan), "finite"), (dict(ambient=inf), "finite"), (dict(background=nan), "finite"), (dict(background=-inf), "finite"),
              (dict(alpha_min=nan), "finite"), (dict(alpha_min=inf), "finite")], [normals, shaded])
    assert l.fenerf_shade_normals(*good.values()) == _lib.OK
    torch.cuda.synchronize()
    assert not bool((normals == PATTERN).any()) and not bool((shaded == PATTERN).any())


# ---- 5. / 6. callers.render_geometry end to end ---------------------------------------------------------------------------------------
# Input chosen on the CPU with the numpy oracle (oracle.fenerf_oracle.render_forward on the draws of _draws(7)): with the FiLM parameters of
# test_mesh_gpu's own seed 4 the density is negative almost everywhere along these rays (8 of 256 rays reach alpha 0.5 from any pose tried), so the
# FiLM parameters are proc.film_params(seed=6).  At yaw pi / 2 + 0.3, pitch pi / 2 - 0.1 the oracle sees 249 of 256 rays visible (alpha >= 0.5),
# 5 of them (2.0 %) with a surface point outside the feature grid's box, none within 2e-5 of a voxel face.
FILM_SEED, DRAW_SEED = 6, 7
YAW, PITCH = math.pi / 2 + 0.3, math.pi / 2 - 0.1
S_, N = 16, 6
KW = dict(img_size=S_, fov=12, ray_start=0.88, ray_end=1.12, num_steps=N, h_stddev=0, v_stddev=0, h_mean=YAW, v_mean=PITCH, hierarchical_sample=True,
          sample_dist=None, clamp_mode="relu", nerf_noise=0, last_back=False, fill_mode="eval_seg_padding_background", fill_color="black")
LIGHT, AMBIENT, BACKGROUND, ALPHA_MIN = (0.3, 0.5, 1.0), 0.25, 1.0, 0.5
# max |grad sigma - fp64 autograd| / max |grad sigma| over the kept visible rays: 1.5 x the value measured on the MI355X (the project's
# convention).  Measured: 2.312e-5 over 244 rays (249 of 256 visible, 5 left out -- the oracle's counts; f16x3 forward-save + fp32 chain +
# input-gradient pass at the 256 surface points; max |grad sigma| 6.6e3, min 1.1e2: the largest angle between the normals is 1.8e-4 rad).
GRAD_REL_MEASURED = 2.312e-5
GRAD_REL_BOUND = 1.5 * GRAD_REL_MEASURED


def _draws(seed):
    """the draws of one hierarchical render without a pose distribution, in _render's order: jitter, coarse noise, u, final noise"""
    R = S_ * S_
    rng = np.random.default_rng(seed)
    return [rng.uniform(0, 1, (1, R, N, 1)).astype(F), rng.normal(size=(1, R, N, 1)).astype(F), rng.uniform(0, 1, (R, N)).astype(F),
            rng.normal(size=(1, R, 2 * N, 1)).astype(F)]


def _with_draws(gen, seed, call):
    gen.draws = VR.RecordedDraws(_draws(seed))
    try:
        out = call()
        assert not gen.draws.arrays, "all recorded draws consumed, in order"
    finally:
        del gen.draws
    return out


def _case():
    gen, mod, spec, sd, _, _ = _generator()
    film = {k: T(v) for k, v in proc.film_params(spec, 1, seed=FILM_SEED).items()}
    meta = dict(truncated_frequencies_geo=film["freq_geo"], truncated_phase_shifts_geo=film["phase_geo"],
                truncated_frequencies_app=film["freq_app"], truncated_phase_shifts_app=film["phase_app"])
    return gen, mod, spec, sd, film, meta


def _unit(light):
    l = np.asarray(light, np.float64)
    return (l / np.linalg.norm(l)).astype(F)


def _check_shading(view, R):
    alpha = view["alpha"].numpy().reshape(1, R)
    wn, ws = E.shade_normals(view["grad"].numpy(), R, alpha, view["cam2world"].numpy(), _unit(LIGHT), AMBIENT, BACKGROUND, ALPHA_MIN)
    assert _same(view["normal"].numpy(), wn.reshape(1, S_, S_, 3).transpose(0, 3, 1, 2)) and _same(view["shaded"].numpy(), ws.reshape(1, 1, S_, S_))
    visible = alpha[0] >= ALPHA_MIN
    length = np.linalg.norm(wn[0].astype(np.float64), axis=-1)
    assert np.abs(length[visible] - 1).max() < 1e-6 and (length[~visible] == 0).all() and (ws[0][~visible] == F(BACKGROUND)).all()
    # the camera frame: the third column of cam2world is the unit vector from the origin to the camera
    c2w, cam = view["cam2world"].numpy()[0].astype(np.float64), view["origins"].numpy()[0, 0].astype(np.float64)
    assert np.abs(c2w.T @ c2w - np.eye(3)).max() < 1e-6 and np.abs(c2w[:, 2] - cam / np.linalg.norm(cam)).max() < 1e-6
    return visible


def test_render_geometry_exact_route_end_to_end():
    from oracle import fenerf_oracle_grad as OG
    from fenerf_amd.siren import autograd as siren_autograd
    gen, mod, spec, sd, film, meta = _case()
    R = S_ * S_
    geo = dict(light=LIGHT, ambient=AMBIENT, background=BACKGROUND, alpha_min=ALPHA_MIN)
    view = _with_draws(gen, DRAW_SEED, lambda: callers.render_geometry(gen, film=meta, details=True, **geo, **KW))
    assert sorted(view) == ["alpha", "cam2world", "depth", "dirs", "grad", "normal", "origins", "pixels", "points", "shaded"]
    assert all(not t.is_cuda for t in view.values()) and all(q.requires_grad for q in mod.parameters())
    assert view["normal"].shape == (1, 3, S_, S_) and view["shaded"].shape == (1, 1, S_, S_) and view["alpha"].shape == (1, S_, S_)
    # pixels and depth: staged_forward_with_frequencies on the same draws, and on the same seed
    staged = lambda: gen.staged_forward_with_frequencies(film["freq_geo"], film["freq_app"], film["phase_geo"], film["phase_app"], **KW)
    px, depth, third = _with_draws(gen, DRAW_SEED, staged)
    assert _same(view["pixels"].numpy(), px.numpy()) and _same(view["depth"].numpy(), depth.numpy())
    assert _same((view["alpha"] * 2 - 1).numpy(), third[:, 0].numpy())          # eval fill mode: `third` is the weight sum
    torch.manual_seed(5)
    seeded = callers.render_geometry(gen, film=meta, **geo, **KW)
    assert sorted(seeded) == ["alpha", "depth", "normal", "pixels", "shaded"]
    torch.manual_seed(5)
    px5, depth5, _ = staged()
    assert _same(seeded["pixels"].numpy(), px5.numpy()) and _same(seeded["depth"].numpy(), depth5.numpy())
    # surface points: the emulation on the render's own rays, depth and weight sum
    o, d = view["origins"].numpy(), view["dirs"].numpy()
    alpha = view["alpha"].numpy().reshape(1, R)
    pts = E.surface_points(o, d, view["depth"].numpy().reshape(1, R), alpha, ALPHA_MIN)
    assert _same(view["points"].numpy(), pts)
    # the gradient: a direct differentiable SIREN call at those points (every weight constant, as extract_mesh's normal route has it)
    params = [q for q in mod.parameters() if q.requires_grad]
    for q in params:
        q.requires_grad_(False)
    try:
        p = T(pts).requires_grad_(True)
        sig = siren_autograd.siren_apply(mod, p, None, film["freq_geo"], film["phase_geo"], film["freq_app"], film["phase_app"])[..., -1]
        g, = torch.autograd.grad(sig.sum(), p)
    finally:
        for q in params:
            q.requires_grad_(True)
    assert _same(view["grad"].numpy(), N_(g))
    # normal and shaded: the shading emulation on that gradient
    visible = _check_shading(view, R)
    assert visible.mean() >= 0.25
    # fp64: grad sigma of the oracle under autograd at the same fp32 points, over the visible rays off the feature grid's voxel faces
    t64 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    sd64 = {k: t64(v) for k, v in sd.items()}
    p64 = t64(pts[:, :R]).requires_grad_(True)
    d64 = torch.zeros((1, R, 3), dtype=torch.float64)
    d64[..., -1] = -1
    f64 = {k: t64(N_(v)) for k, v in film.items()}
    OG.siren_forward(sd64, spec, p64, d64, f64["freq_geo"], f64["phase_geo"], f64["freq_app"], f64["phase_app"])[..., -1].sum().backward()
    ref = p64.grad[0].numpy()
    gi = (pts[0, :R].astype(np.float64) * (2 / 0.24) + 1) / 2 * (GRID - 1)
    left_out = (np.abs(gi - np.round(gi)) < 2e-5).any(-1) | (np.abs(pts[0, :R]) > 0.12).any(-1)
    keep = visible & ~left_out
    assert (visible & left_out).sum() <= 0.05 * visible.sum()
    got = view["grad"].numpy()[0, :R].astype(np.float64)
    rel = float(np.abs(got[keep] - ref[keep]).max() / np.abs(ref[keep]).max())
    cos = (got[keep] * ref[keep]).sum(-1) / (np.linalg.norm(got[keep], axis=-1) * np.linalg.norm(ref[keep], axis=-1))
    print(f"[geometry] exact route {S_}x{S_}, {N}+{N}: {int(visible.sum())} of {R} rays visible, {int((visible & left_out).sum())} left out; grad sigma vs fp64 "
          f"autograd over {int(keep.sum())} rays: max-norm relative error {rel:.3e}, largest normal angle {float(np.arccos(np.clip(cos, -1, 1)).max()):.3e} rad, "
          f"max |grad sigma| {np.abs(ref[keep]).max():.3e}, min |grad sigma| {np.linalg.norm(ref[keep], axis=-1).min():.3e}")
    assert rel <= GRAD_REL_BOUND          # measured 2.312e-5
    # world space: the same normals before the rotation; no-grad only
    world = _with_draws(gen, DRAW_SEED, lambda: callers.render_geometry(gen, film=meta, space="world", details=True, **geo, **KW))
    assert world["cam2world"] is None
    wn, _ = E.shade_normals(world["grad"].numpy(), R, alpha, None, _unit(LIGHT), AMBIENT, BACKGROUND, ALPHA_MIN)
    assert _same(world["grad"].numpy(), view["grad"].numpy()) and _same(world["normal"].numpy(), wn.reshape(1, S_, S_, 3).transpose(0, 3, 1, 2))
    with pytest.raises(RuntimeError):
        callers.render_geometry(gen, film=dict(meta, truncated_frequencies_geo=film["freq_geo"].clone().requires_grad_(True)), **KW)
    with pytest.raises(ValueError):
        callers.render_geometry(gen, film=meta, space="object", **KW)


def test_render_geometry_baked_route_end_to_end():
    gen, mod, spec, sd, film, meta = _case()
    R = S_ * S_
    geo = dict(light=LIGHT, ambient=AMBIENT, background=BACKGROUND, alpha_min=ALPHA_MIN)
    cube = callers.baked_cube_length(KW["fov"], KW["ray_start"], KW["ray_end"], num_steps=N)
    field = callers.bake_field(gen, None, film=meta, resolution=24, cube_length=cube)
    view = _with_draws(gen, DRAW_SEED, lambda: callers.render_geometry(gen, baked=field, details=True, **geo, **KW))
    px, depth, _ = _with_draws(gen, DRAW_SEED, lambda: field.render(gen, **KW))
    assert _same(view["pixels"].numpy(), px.numpy()) and _same(view["depth"].numpy(), depth.numpy())
    alpha = view["alpha"].numpy().reshape(1, R)
    pts = E.surface_points(view["origins"].numpy(), view["dirs"].numpy(), view["depth"].numpy().reshape(1, R), alpha, ALPHA_MIN)
    assert _same(view["points"].numpy(), pts)
    g = E.volume_sample_grad(N_(field.vol), field.origin, field.spacing, pts.reshape(-1, 3), field.C - 1).reshape(pts.shape)
    assert _same(view["grad"].numpy(), g) and (g != 0).any()
    visible = _check_shading(view, R)
    # a resolution instead of a field: the same lattice, the same view
    by_res = _with_draws(gen, DRAW_SEED, lambda: callers.render_geometry(gen, film=meta, baked=24, **geo, **KW))
    assert all(_same(by_res[k].numpy(), view[k].numpy()) for k in by_res)
    # against the exact route (printed, not asserted: the size of the approximation depends on the field)
    exact = _with_draws(gen, DRAW_SEED, lambda: callers.render_geometry(gen, film=meta, **geo, **KW))
    both = visible & (exact["alpha"].numpy().reshape(R) >= ALPHA_MIN)
    nb, ne = (v["normal"].numpy()[0].reshape(3, R).T.astype(np.float64)[both] for v in (view, exact))
    angle = np.arccos(np.clip((nb * ne).sum(-1), -1, 1))
    print(f"[geometry] baked 24^3 vs exact normals, {S_}x{S_}: mean angle {angle.mean():.3e} rad, 95th percentile {np.quantile(angle, 0.95):.3e} rad over "
          f"{int(both.sum())} rays visible in both; max |shaded difference| {float((view['shaded'] - exact['shaded']).abs().max()):.3e}")


def test_video_caller_geometry_frames_beside_the_unchanged_ones():
    gen, mod, spec, sd, film, meta = _case()
    options = {k: v for k, v in KW.items() if k not in ("h_mean", "v_mean")}
    trajectory = [(0.0, PITCH, YAW, 12), (1.0, PITCH + 0.05, YAW - 0.1, 12)]
    plain = callers.render_double_latent_video(gen, 3, options, trajectory, latent_type="geo", psi=0.7)
    geo = callers.render_double_latent_video(gen, 3, options, trajectory, latent_type="geo", psi=0.7, geometry=dict(light=LIGHT))
    assert sorted(plain) == ["acc", "depth", "images", "labels"] and sorted(geo) == ["acc", "depth", "images", "labels", "normal", "shaded"]
    for k in plain:          # the same seeds, the same draws: the same frames
        assert _same(geo[k].numpy(), plain[k].numpy()), k
    assert geo["normal"].shape == (2, 3, S_, S_) and geo["shaded"].shape == (2, 1, S_, S_)
    length = geo["normal"].double().norm(dim=1)
    assert bool(((length - 1).abs() < 1e-6).logical_or(length == 0).all()) and bool((length > 0).any())


# ---- 7. the tool --------------------------------------------------------------------------------------------------------------------
def test_render_multiview_tool_writes_the_geometry_images(tmp_path):
    from PIL import Image
    g = load_golden("tiny_multiview")
    cur = json.loads(str(g["curriculum_json"]))
    cur.update(output_dim=22, eval_last_back=False)
    cur_file = str(tmp_path / "tiny_curriculum.json")
    json.dump(cur, open(cur_file, "w"))
    base = [sys.executable, os.path.join(ROOT, "tools", "render_multiview.py"), os.path.join(GOLDEN, "ref_generator_tiny.pth"), "--no_ema", "--curriculum", cur_file,
            "--seeds", "3", "--image_size", "16", "--ray_step_multiplier", "1"]
    plain, geo = str(tmp_path / "plain"), str(tmp_path / "geo")
    for out, extra in ((plain, []), (geo, ["--geometry", "--light", "0.3", "0.5", "1", "--ambient", "0.2"])):
        r = subprocess.run(base + ["--output_dir", out] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert sorted(os.listdir(plain)) == ["grid_3_RGB.png", "grid_3_SEG.png"]
    assert sorted(os.listdir(geo)) == ["grid_3_RGB.png", "grid_3_SEG.png", "grid_3_normal.png", "grid_3_shaded.png"]
    for name in ("grid_3_normal.png", "grid_3_shaded.png"):
        assert np.asarray(Image.open(os.path.join(geo, name))).shape == (16 + 4, 5 * 18 + 2, 3)          # five 16 x 16 views, padding 2
    for name in ("grid_3_RGB.png", "grid_3_SEG.png"):          # the render itself is the same
        assert np.array_equal(np.asarray(Image.open(os.path.join(geo, name))), np.asarray(Image.open(os.path.join(plain, name))))
