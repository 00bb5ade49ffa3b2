"""Camera-pose gradients through the differentiable render: fenerf_ray_grads, fenerf_render_backward_rays, the autograd nodes, the
generator API and callers.inverse_render(optimize_pose=True), against numpy / torch fp64 restatements.

Semantics under test (include/fenerf.h): sample depths are constants of the graph; with p = o + d z,
    d_origins = sum_pass sum_n d_points,    d_dirs = sum_pass sum_n z d_points + (locked view ? 0 : sum_pass sum_n d_viewdirs)."""
import functools
import math
import os

import numpy as np
import pytest
import torch

from test_gpu_parity import DEV, N_, PRECISIONS, T, _rel_err, _siren_module, proc
from fenerf_amd import _lib, native
from fenerf_amd.generators import autograd as GA
from fenerf_amd.generators import generators as G
from fenerf_amd.generators import volumetric_rendering as VR
from fenerf_amd.siren import autograd as SA
from fenerf_amd.siren import siren as S

pytestmark = pytest.mark.gpu

# Relative error (max |got - ref| / max |ref|) of d_origins / d_dirs against fp64 autograd, per precision: 1.5 x the worst value measured
# on the MI355X over the cases of the test that asserts it (the project's convention; profiles/r09_pose_grads.md has the measurements).
# Measured worst (d_origins, d_dirs over models, shapes, weight-gradient and FiLM-only steps): f32 2.89e-5, f16x3 8.95e-5, tape16 1.64e-4.
RAY_GRAD_BOUND = {"f32": 1.5 * 2.89e-5, "f16x3": 1.5 * 8.95e-5, "tape16": 1.5 * 1.64e-4}
# |yaw.grad - ref| / |ref| (and pitch) of the generator-level test against the fp64 chain, 1.5 x the worst measured over its cases: f32 5.28e-4,
# f16x3 6.55e-4 (both on the hierarchical render at the fixed pose, where the yaw gradient is a small difference of large per-ray terms:
# -0.62 against +-45 in the other cases, which sit at 1e-5 - 4e-4)
POSE_GRAD_BOUND = {"f32": 1.5 * 5.28e-4, "f16x3": 1.5 * 6.55e-4}


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. the reduction alone
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,R,N,passes", [(2, 5, 3, 2), (1, 3, 64, 2), (1, 2, 512, 1)])
def test_ray_grads_kernel_vs_fp64_sum(B, R, N, passes):
    """fenerf_ray_grads against a numpy fp64 sum of random per-sample inputs.  (2, 5, 3): 15 points per image padded to 32 -- pad rows and
    image offsets; with and without d_viewdirs; each output NULL in turn.  Bound per element (derived, not measured): the sum of at most
    2 * passes * N <= 4 N terms (products rounded once: FMAs), each partial sum rounded once: |err| <= 4 N 2^-24 sum |terms|.  NaN in
    the pad rows must not reach any output; a NaN in one real sample makes exactly that ray's sums NaN."""
    rng = np.random.default_rng(B * 1000 + N)
    P, Pp = R * N, (R * N + 31) // 32 * 32
    dp = rng.normal(size=(passes * B, Pp, 3)).astype(np.float32)
    dv = rng.normal(size=(passes * B, Pp, 3)).astype(np.float32)
    dp[:, P:], dv[:, P:] = np.nan, np.nan
    zc = rng.uniform(0.88, 1.12, (B, R, N)).astype(np.float32)
    zf = rng.uniform(0.88, 1.12, (B, R, N)).astype(np.float32) if passes == 2 else None
    z = np.stack([zc, zf] if passes == 2 else [zc]).astype(np.float64)                                   # [passes,B,R,N]

    def reference(dp, dv):
        p64 = dp[:, :P].astype(np.float64).reshape(passes, B, R, N, 3)
        o = p64.sum((0, 3))
        d = (p64 * z[..., None]).sum((0, 3))
        mo, md = np.abs(p64).sum((0, 3)), np.abs(p64 * z[..., None]).sum((0, 3))
        if dv is not None:
            v64 = dv[:, :P].astype(np.float64).reshape(passes, B, R, N, 3)
            d, md = d + v64.sum((0, 3)), md + np.abs(v64).sum((0, 3))
        return o, d, mo, md

    eps = 4 * N * 2.0 ** -24
    for use_dv in (True, False):
        ref_o, ref_d, mag_o, mag_d = reference(dp, dv if use_dv else None)
        for want_o, want_d in ((True, True), (True, False), (False, True)):
            got_o, got_d = native.ray_grads(T(dp), T(dv) if use_dv else None, T(zc), T(zf) if zf is not None else None, want_o, want_d)
            assert (got_o is None) == (not want_o) and (got_d is None) == (not want_d)
            if want_o:
                assert got_o.shape == (B, R, 3) and np.isfinite(N_(got_o)).all(), "pad rows are never read"
                assert (np.abs(N_(got_o) - ref_o) <= eps * mag_o).all(), float((np.abs(N_(got_o) - ref_o) / mag_o).max())
            if want_d:
                assert got_d.shape == (B, R, 3) and np.isfinite(N_(got_d)).all()
                assert (np.abs(N_(got_d) - ref_d) <= eps * mag_d).all(), float((np.abs(N_(got_d) - ref_d) / mag_d).max())
    # run to run: the same bits
    a = native.ray_grads(T(dp), T(dv), T(zc), T(zf) if zf is not None else None)
    b = native.ray_grads(T(dp), T(dv), T(zc), T(zf) if zf is not None else None)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # one non-finite real sample: plain sums, no filtering -- that ray and no other
    b_, r_, n_ = B - 1, R // 2, N - 1
    dp2 = dp.copy()
    dp2[(passes - 1) * B + b_, r_ * N + n_, 1] = np.nan
    got_o, got_d = native.ray_grads(T(dp2), T(dv), T(zc), T(zf) if zf is not None else None)
    nan_o, nan_d = np.isnan(N_(got_o)), np.isnan(N_(got_d))
    want = np.zeros((B, R, 3), bool)
    want[b_, r_, 1] = True
    assert np.array_equal(nan_o, want) and np.array_equal(nan_d, want)
    with pytest.raises(_lib.FenerfError, match="both NULL"):
        native.ray_grads(T(dp), T(dv), T(zc), T(zf) if zf is not None else None, False, False)


# ------------------------------------------------------------------------------------------------------------------------------------
# the hierarchical node on explicit rays
# ------------------------------------------------------------------------------------------------------------------------------------
MODELS = {"texture": ("texture", 32, 5, False), "baseline_lock": ("baseline", 64, 0, True),
          # the texture model with the three view-direction columns of colour layer 0 scaled by VIEW_GAIN: in the models above the
          # view-direction sum is 2e-5 - 2e-4 of d_dirs (d_points carries the box warp's 2 / 0.24 and eleven layers of frequencies ~ 30, the
          # view direction enters one colour layer), i.e. below the fp32-class error of d_dirs itself, whatever the seeds -- so that a
          # gradient without that term is told apart here
          "texture_view": ("texture", 32, 5, False)}
VIEW_GAIN = 1000.0
SHAPES = {"aligned": (2, 8, 8, 0), "ragged": (2, 7, 11, 128)}          # B, img_size, N, chunk_points (0 = default)


@functools.lru_cache(maxsize=None)
def _inputs(B, S_, N, seed=11):
    """rays of two random poses, jittered depths and the render's draws -- computed once, never modified"""
    R = S_ * S_
    torch.manual_seed(seed)
    origins, dirs, z, _, _ = VR.sample_rays(B, N, torch.device(DEV), 12, (S_, S_), 0.88, 1.12, 0.3, 0.155, math.pi / 2, math.pi / 2, "gaussian")
    u = torch.rand((B * R, N), device=DEV)
    noise_c, noise_f = torch.randn((B * R, N), device=DEV), torch.randn((B * R, 2 * N), device=DEV)
    w = torch.randn((B, R, 21), device=DEV)
    return origins, dirs, z.reshape(B, R, N), u, noise_c, noise_f, w


def _run_node(mod, spec, shape, lock_view, film_only=False, rays=True, abi=True, chunk=None, det=None):
    """One forward + backward of HierarchicalRenderFunction on the shared inputs -> dict of numpy results"""
    B, S_, N, chunk0 = SHAPES[shape]
    origins, dirs, z_c, u, noise_c, noise_f, w = _inputs(B, S_, N)
    o, d = origins.clone().requires_grad_(rays), dirs.clone().requires_grad_(rays)
    film = {k: T(v).requires_grad_(True) for k, v in proc.film_params(spec, B, seed=4).items()}
    for p_ in mod.parameters():
        p_.requires_grad_(not film_only)
        p_.grad = None
    opts, copts = _lib.composite_opts("relu", 0.2), _lib.composite_opts("relu", 0.2)
    old = (SA.BACKWARD_CHUNK_POINTS, GA.USE_RENDER_ABI, mod.deterministic_backward)
    SA.BACKWARD_CHUNK_POINTS, GA.USE_RENDER_ABI, mod.deterministic_backward = (chunk if chunk is not None else (chunk0 or old[0])), abi, det
    try:
        with native.phase_timing() as t:
            rgb, _ = GA.HierarchicalRenderFunction.apply(mod, opts, copts, lock_view, o, d, z_c, u, noise_c, noise_f, film["freq_geo"], film["phase_geo"],
                                                         film["freq_app"], film["phase_app"], *mod._render_params())
            (rgb * w).sum().backward()
    finally:
        SA.BACKWARD_CHUNK_POINTS, GA.USE_RENDER_ABI, mod.deterministic_backward = old
    g = {k: N_(v.grad) for k, v in film.items()}
    g.update({k: N_(p_.grad) for k, p_ in mod.named_parameters() if p_.grad is not None})
    return dict(rgb=N_(rgb), grads=g, d_o=N_(o.grad) if rays else None, d_d=N_(d.grad) if rays else None, calls=dict(t.calls))


@functools.lru_cache(maxsize=None)
def _module(model, precision):
    kind, H, grid, lock = MODELS[model]
    mod, spec, sd = _siren_module(kind, H, grid, sigma_gain=150.0, precision=precision)
    if model == "texture_view":
        sd = dict(sd)
        sd["color_layer_sine.0.layer.weight"] = sd["color_layer_sine.0.layer.weight"].copy()
        sd["color_layer_sine.0.layer.weight"][:, :3] *= VIEW_GAIN                                    # columns [dirs 3 | grid features | x]
        with torch.no_grad():
            mod.color_layer_sine[0].layer.weight[:, :3] *= VIEW_GAIN
    return mod, spec, sd, lock


@functools.lru_cache(maxsize=None)
def _fp64_ray_grads(model, shape):
    """fp64 autograd of the restatement (oracle.fenerf_oracle_grad) on the same rays, with the coarse depths and the native forward's
    resampled depths teacher-forced -> the ray gradients, and the same with one term dropped at a time."""
    from oracle import fenerf_oracle_grad as OG
    mod, spec, sd, lock = _module(model, "f32")
    B, S_, N, _ = SHAPES[shape]
    R = S_ * S_
    origins, dirs, z_c, u, noise_c, noise_f, w = _inputs(B, S_, N)
    film = proc.film_params(spec, B, seed=4)
    nat = mod.native_differentiable(DEV)
    with torch.no_grad():
        pts_c = (origins.unsqueeze(2) + dirs.unsqueeze(2) * z_c.unsqueeze(-1)).reshape(B, R * N, 3)
        rd = None if lock else dirs.unsqueeze(2).expand(-1, -1, N, -1).reshape(B, R * N, 3).contiguous()
        coarse = nat.siren_forward(pts_c, rd, *(T(film[k]) for k in ("freq_geo", "phase_geo", "freq_app", "phase_app")))
        _, _, w_c, _ = native.composite(coarse.reshape(B * R, N, 22), z_c.reshape(B * R, N), noise_c, _lib.composite_opts("relu", 0.2), want_wsum=False)
        z_f = native.resample(z_c.reshape(B * R, N), w_c, u).reshape(B, R, N)
    t64 = lambda a: torch.as_tensor(N_(a) if torch.is_tensor(a) else np.asarray(a), dtype=torch.float64)
    sd64 = {k: t64(v) for k, v in sd.items()}
    args = tuple(t64(film[k]) for k in ("freq_geo", "phase_geo", "freq_app", "phase_app"))
    o64, d64 = t64(origins).requires_grad_(True), t64(dirs).requires_grad_(True)
    zc64, zf64 = t64(z_c), t64(z_f)
    locked = torch.zeros((B, R * N, 3), dtype=torch.float64)
    locked[..., -1] = -1                                                                                # generators.py:477-479
    pts, rds, rows = [], [], []
    for z64 in (zc64, zf64):
        p = (o64.unsqueeze(2) + d64.unsqueeze(2) * z64.unsqueeze(-1)).reshape(B, R * N, 3)
        v = locked if lock else d64.unsqueeze(2).expand(-1, -1, N, -1).reshape(B, R * N, 3)
        p.retain_grad()
        if not lock:
            v.retain_grad()
        pts.append(p); rds.append(v)
        rows.append(OG.siren_forward(sd64, spec, p, v, *args))
    rgb, _, _ = OG.merge_composite(rows[1].reshape(B * R, N, 22), rows[0].reshape(B * R, N, 22), zf64.reshape(B * R, N), zc64.reshape(B * R, N),
                                   t64(noise_f), noise_std=0.2, clamp_mode="relu")
    (rgb.reshape(B, R, 21) * t64(w)).sum().backward()
    dp = np.stack([p.grad.numpy().reshape(B, R, N, 3) for p in pts])                                    # [2,B,R,N,3]
    dv = np.zeros_like(dp) if lock else np.stack([v.grad.numpy().reshape(B, R, N, 3) for v in rds])
    z = np.stack([zc64.numpy(), zf64.numpy()])[..., None]
    full = (dp.sum((0, 3)), (z * dp).sum((0, 3)) + dv.sum((0, 3)))
    # the formulas of include/fenerf.h ARE autograd's broadcast sums
    assert np.abs(full[0] - o64.grad.numpy()).max() <= 1e-12 * np.abs(full[0]).max()
    assert np.abs(full[1] - d64.grad.numpy()).max() <= 1e-12 * np.abs(full[1]).max()
    dropped = {"z factor": (full[0], dp.sum((0, 3)) + dv.sum((0, 3))),
               "fine pass": (dp[0].sum(2), (z[0] * dp[0]).sum(2) + dv[0].sum(2))}
    if not lock:
        dropped["view-direction sum"] = (full[0], (z * dp).sum((0, 3)))
    return full, dropped


@pytest.mark.parametrize("precision", PRECISIONS + ["tape16"])
@pytest.mark.parametrize("film_only", [False, True], ids=["weights", "film_only"])
@pytest.mark.parametrize("model,shape", [("texture", "aligned"), ("texture", "ragged"), ("baseline_lock", "aligned"), ("baseline_lock", "ragged"),
                                         ("texture_view", "ragged")])
def test_render_backward_rays_vs_fp64_autograd(model, shape, film_only, precision):
    """fenerf_render_backward_rays (through HierarchicalRenderFunction with origins / dirs that require grad) against fp64 autograd of
    oracle.fenerf_oracle_grad on points built as o + d z.  texture H = 32 with a 5^3 grid, and the baseline H = 64 without a grid under a
    locked view; sigma_gain 150, nerf_noise 0.2, relu clamp; 2 x 8 x 8 x 8 (512 points per pass: whole tiles, one chunk) and 2 x 7 x 7 x 11
    (539 -> 544 points, 128-point chunks: rays straddle tiles, chunk boundaries and the pass boundary); weight-gradient and FiLM-only steps.
    Measured on the MI355X (worst over models, shapes and step kinds; max |err| / max |ref|):
        f32 2.89e-5 (texture, aligned), f16x3 8.95e-5, tape16 1.64e-4 (both baseline, aligned, weight-gradient step); the full table is
        in profiles/r09_pose_grads.md.  Asserted: 1.5 x these (RAY_GRAD_BOUND).
    The bound must also separate the gradient from the same gradient with one term dropped (the z factor, the view-direction sum, the
    fine pass): every asserted bound is below a third of the smallest of those distances."""
    mod, spec, sd, lock = _module(model, precision)
    full, dropped = _fp64_ray_grads(model, shape)
    r = _run_node(mod, spec, shape, lock, film_only=film_only)
    e_o, e_d = _rel_err(r["d_o"], full[0]), _rel_err(r["d_d"], full[1])
    dist = {k: min(_rel_err(v[0], full[0]) if not np.array_equal(v[0], full[0]) else np.inf, _rel_err(v[1], full[1])) for k, v in dropped.items()}
    print(f"[pose] ray gradients vs fp64 [{model}, {shape}, {'film-only' if film_only else 'weights'}, {precision}]: d_origins {e_o:.2e} d_dirs {e_d:.2e}; "
          f"distance of the gradient with a term dropped: " + ", ".join(f"{k} {v:.2e}" for k, v in dist.items()))
    assert np.isfinite(r["d_o"]).all() and np.isfinite(r["d_d"]).all() and np.abs(full[0]).max() > 0 and np.abs(full[1]).max() > 0
    # (the view-direction sum of the plain texture model is below fp32 resolution of d_dirs -- see MODELS; "texture_view" asserts that term)
    asserted = {k: v for k, v in dist.items() if not (model == "texture" and k == "view-direction sum")}
    assert model != "texture_view" or "view-direction sum" in asserted
    assert min(asserted.values()) >= 1e-2, dist
    bound = RAY_GRAD_BOUND[precision]
    assert bound is not None, "no measured bound recorded"
    assert bound <= min(asserted.values()) / 3, (bound, dist)
    assert e_o <= bound and e_d <= bound, (e_o, e_d, bound)


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. nothing else moves
# ------------------------------------------------------------------------------------------------------------------------------------
def _same_grads(a, b, exact_grid):
    assert a.keys() == b.keys()
    for k in a:
        if k == "spatial_embeddings" and not exact_grid:      # fp32 atomics: the order of the sum varies from run to run
            assert _rel_err(a[k], b[k]) <= 1e-6, (k, _rel_err(a[k], b[k]))
        else:
            assert np.array_equal(a[k], b[k]), (k, _rel_err(a[k], b[k]))


@pytest.mark.parametrize("precision", PRECISIONS + ["tape16"])
@pytest.mark.parametrize("model,shape", [("texture", "ragged"), ("baseline_lock", "aligned")])
def test_ray_gradients_leave_every_other_gradient_alone(model, shape, precision):
    """With ray gradients requested on a weight-gradient step, pixels and every weight / grid / FiLM gradient are those of
    fenerf_render_backward on the same inputs bit for bit (the atomically scattered grid gradient to 1e-6; bit for bit in the
    deterministic mode); the C-ABI call and the Python orchestration (chunked_backward(input_grads=...) + native.ray_grads) deliver
    the same d_origins / d_dirs bit for bit; so do two runs."""
    mod, spec, sd, lock = _module(model, precision)
    plain = _run_node(mod, spec, shape, lock, rays=False)
    rays = _run_node(mod, spec, shape, lock, rays=True)
    assert np.array_equal(plain["rgb"], rays["rgb"])
    _same_grads(plain["grads"], rays["grads"], exact_grid=False)
    assert len(rays["grads"]) > 30 and rays["calls"].get("chain", 0) == plain["calls"].get("chain", 0) >= 1
    again = _run_node(mod, spec, shape, lock, rays=True)
    assert np.array_equal(rays["d_o"], again["d_o"]) and np.array_equal(rays["d_d"], again["d_d"]), "run to run"
    py = _run_node(mod, spec, shape, lock, rays=True, abi=False)
    assert np.array_equal(py["rgb"], rays["rgb"])
    assert np.array_equal(py["d_o"], rays["d_o"]) and np.array_equal(py["d_d"], rays["d_d"]), "C-ABI call vs Python orchestration"
    _same_grads(py["grads"], rays["grads"], exact_grid=False)
    if spec["grid_ch"]:
        det_plain = _run_node(mod, spec, shape, lock, rays=False, det=True)
        det_rays = _run_node(mod, spec, shape, lock, rays=True, det=True)
        _same_grads(det_plain["grads"], det_rays["grads"], exact_grid=True)
        assert np.array_equal(det_rays["d_o"], rays["d_o"]) and np.array_equal(det_rays["d_d"], rays["d_d"])


@pytest.mark.parametrize("precision", PRECISIONS + ["tape16"])
def test_ray_gradients_do_not_depend_on_the_chunking(precision):
    """d_origins / d_dirs for backward chunks of 128 points, of 1700 and the default (one chunk) are the same bits: per-sample gradients
    are per-tile quantities, chunk boundaries fall on multiples of 128 points, and the reduction walks a ray in a fixed order."""
    mod, spec, sd, lock = _module("texture", precision)
    res = [_run_node(mod, spec, "ragged", lock, chunk=c) for c in (128, 1700, SA.BACKWARD_CHUNK_POINTS)]
    assert res[0]["calls"].get("chain", 0) > res[1]["calls"].get("chain", 0) > res[2]["calls"].get("chain", 0) >= 1
    for r in res[1:]:
        assert np.array_equal(r["d_o"], res[0]["d_o"]) and np.array_equal(r["d_d"], res[0]["d_d"])


def test_film_only_f16x3_step_with_ray_gradients():
    """The FiLM-only step of an f16x3 model loses its no-dump chain while ray gradients are on (the input-gradient pass reads the dump):
    its FiLM gradients are then the dumping chain's -- within the bound that route's own test holds the two chains to (1e-5 on the phase
    gradients, 2e-4 on the frequency gradients) of the step without ray gradients; C-ABI call and Python orchestration agree bit for bit."""
    mod, spec, sd, lock = _module("texture", "f16x3")
    plain = _run_node(mod, spec, "ragged", lock, film_only=True, rays=False)
    rays = _run_node(mod, spec, "ragged", lock, film_only=True, rays=True)
    assert np.array_equal(plain["rgb"], rays["rgb"]) and sorted(rays["grads"]) == sorted(plain["grads"]) and len(rays["grads"]) == 4
    for k in plain["grads"]:
        assert _rel_err(rays["grads"][k], plain["grads"][k]) <= (1e-5 if "phase" in k else 2e-4), (k, _rel_err(rays["grads"][k], plain["grads"][k]))
    py = _run_node(mod, spec, "ragged", lock, film_only=True, rays=True, abi=False)
    assert np.array_equal(py["d_o"], rays["d_o"]) and np.array_equal(py["d_d"], rays["d_d"])
    _same_grads(py["grads"], rays["grads"], exact_grid=True)


def test_render_backward_rays_refusals():
    """both outputs NULL is invalid; AMP-class models (bf16 dumps) are refused by the library and, up front, by the autograd node"""
    mod, spec, sd, lock = _module("texture", "f16x3")
    B, S_, N, _ = SHAPES["aligned"]
    origins, dirs, z_c, u, noise_c, noise_f, w = _inputs(B, S_, N)
    nat = mod.native_differentiable(DEV)
    film = [T(v) for v in (proc.film_params(spec, B, seed=4)[k] for k in ("freq_geo", "phase_geo", "freq_app", "phase_app"))]
    opts = _lib.composite_opts("relu", 0.2)
    rgb, _, save = nat.render_forward_save(origins, dirs, z_c, u, noise_c, noise_f, *film, opts)
    w_geo, w_col = SA.film_layer_weights(mod, mod._render_params())
    with pytest.raises(ValueError, match="neither"):
        nat.render_backward(B, S_ * S_, N, save, z_c, noise_f, opts, w.contiguous(), True, ray_grads=(w_geo[0], w_col[0], False, False))
    l = _lib.lib()
    import ctypes as C
    g = _lib.FenerfSirenGrads()
    p = C.c_void_p(save.data_ptr())
    rc = l.fenerf_render_backward_rays(nat._h, B, S_ * S_, N, 0, p, save.numel(), 0, p, None, C.byref(opts), p, C.byref(g), None, None, 0, 0, p, 16, p, p, 35,
                                       None, None, None)
    assert rc == _lib.E_INVALID and "both NULL" in l.fenerf_last_error().decode()
    amp, spec_a, _ = _siren_module("texture", 32, 5, sigma_gain=150.0)
    amp.grad_precision = "amp"
    o, d = origins.clone().requires_grad_(True), dirs.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="grad_precision"):
        GA.HierarchicalRenderFunction.apply(amp, opts, opts, False, o, d, z_c, u, noise_c, noise_f, *film, *amp._render_params())


# ------------------------------------------------------------------------------------------------------------------------------------
# 4. the generator API: h_mean / v_mean as tensors that require grad
# ------------------------------------------------------------------------------------------------------------------------------------
def _double_generator(mod):
    gen = G.DoubleImplicitGenerator3d(functools.partial(S.TextureEmbeddingPiGAN128SEMANTICDISENTANGLE, hidden_dim=32), 8, 8, 22)
    gen.siren = mod
    gen = gen.to(DEV)
    gen.device = torch.device(DEV); gen.siren.device = gen.device
    return gen


YAW0, PITCH0 = math.pi / 2 + 0.1, math.pi / 2 - 0.07


def _pose_kw(S_, N, hier, spread):
    return dict(img_size=S_, fov=12, ray_start=0.88, ray_end=1.12, num_steps=N, h_stddev=0.3 if spread else 0, v_stddev=0.155 if spread else 0,
                hierarchical_sample=hier, sample_dist="gaussian" if spread else None, clamp_mode="relu", nerf_noise=0.2, last_back=False)


def _render_with_pose(gen, spec, B, kw, seed=11, pose_grad=True, film_grad=True):
    """-> (pixels, poses, yaw, pitch, film tensors) of one seeded forward_with_frequencies with the pose as 0-dim tensors (or floats)"""
    film = {k: T(v).requires_grad_(film_grad) for k, v in proc.film_params(spec, B, seed=4).items()}
    yaw = torch.tensor(YAW0, dtype=torch.float32, device=DEV, requires_grad=True) if pose_grad else YAW0
    pitch = torch.tensor(PITCH0, dtype=torch.float32, device=DEV, requires_grad=True) if pose_grad else PITCH0
    torch.manual_seed(seed)
    px, poses = gen.forward_with_frequencies(film["freq_geo"], film["freq_app"], film["phase_geo"], film["phase_app"], h_mean=yaw, v_mean=pitch, **kw)
    return px, poses, yaw, pitch, film


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("spread", [False, True], ids=["fixed_pose", "gaussian_pose"])
@pytest.mark.parametrize("hier", [True, False], ids=["hierarchical", "single_pass"])
def test_generator_pose_gradient_vs_fp64_chain(hier, spread, precision):
    """forward_with_frequencies with h_mean / v_mean as 0-dim tensors that require grad: the image is that of the same seeded call with
    plain numbers bit for bit, the returned poses carry the graph, and yaw.grad / pitch.grad equal fp64 autograd of the whole chain -- fp64
    torch rays from the same draws -> points o + d z (coarse and, teacher-forced, the native forward's resampled depths) -> the oracle's
    SIREN -> composite -> (img * w).sum().  Hierarchical (one node, fenerf_render_backward_rays) and single-pass (SirenFunction's input
    gradients + torch's broadcast sums).  Measured on the MI355X (relative error of yaw.grad / pitch.grad): hierarchical, fixed pose f32
    5.28e-4 / 4.74e-4, f16x3 6.55e-4 / 4.16e-4; hierarchical, gaussian pose f32 1.06e-4 / 8.57e-5, f16x3 3.71e-4 / 1.16e-4; single pass
    1.0e-5 - 2.0e-5 in every case.  Asserted: 1.5 x the worst per precision (POSE_GRAD_BOUND)."""
    from oracle import fenerf_oracle_grad as OG
    mod, spec, sd = _siren_module("texture", 32, 5, sigma_gain=150.0, precision=precision)
    gen = _double_generator(mod)
    B, S_, N = 2, 6, 8
    R, M = S_ * S_, (2 * N if hier else N)
    kw = _pose_kw(S_, N, hier, spread)
    px, poses, yaw, pitch, _ = _render_with_pose(gen, spec, B, kw)
    px_plain, poses_plain, _, _, _ = _render_with_pose(gen, spec, B, kw, pose_grad=False)
    assert torch.equal(px, px_plain) and torch.equal(poses, poses_plain), "bit-identical to the call with plain numbers"
    assert poses.requires_grad and px.requires_grad
    w = torch.randn(px.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    (px * w).sum().backward()
    assert yaw.grad is not None and pitch.grad is not None and yaw.grad.shape == () and pitch.grad.shape == ()
    # ---- replay of the draws: the constants of the graph from the native pieces, the camera angles in fp64
    dev = gen.device
    torch.manual_seed(11)
    origins, dirs, z_vals, _, _ = VR.sample_rays(B, N, dev, 12, (S_, S_), 0.88, 1.12, kw["h_stddev"], kw["v_stddev"], YAW0, PITCH0, kw["sample_dist"], draws=gen.draws)
    noise_c = u = None
    if hier:
        noise_c, u = gen.draws.randn((B, R, N, 1), dev), gen.draws.rand((B * R, N), dev)
    noise_f = gen.draws.randn((B, R, M, 1), dev)
    torch.manual_seed(11)
    gen.draws.rand((B, R, N, 1), dev)
    t64 = lambda a: torch.as_tensor(N_(a) if torch.is_tensor(a) else np.asarray(a), dtype=torch.float64)
    y64 = torch.tensor(float(np.float32(YAW0)), dtype=torch.float64, requires_grad=True)
    p64 = torch.tensor(float(np.float32(PITCH0)), dtype=torch.float64, requires_grad=True)
    if spread:
        theta = t64(gen.draws.randn((B, 1), dev)) * kw["h_stddev"] + y64
        phi = t64(gen.draws.randn((B, 1), dev)) * kw["v_stddev"] + p64
    else:
        theta, phi = torch.ones((B, 1), dtype=torch.float64) * y64, torch.ones((B, 1), dtype=torch.float64) * p64
    o64, d64, _, _ = VR.rays_from_angles(theta, phi, (S_, S_), 12, "cpu")
    assert float((o64.detach() - t64(origins)).abs().max()) <= 1e-6 and float((d64.detach() - t64(dirs)).abs().max()) <= 1e-6
    z_c = z_vals.reshape(B, R, N)
    film = proc.film_params(spec, B, seed=4)
    copts = _lib.composite_opts("relu", 0.2)
    depths = [t64(z_c)]
    if hier:
        nat = mod.native_differentiable(DEV)
        with torch.no_grad():
            pts_c = (origins.unsqueeze(2) + dirs.unsqueeze(2) * z_c.unsqueeze(-1)).reshape(B, R * N, 3)
            rd = dirs.unsqueeze(2).expand(-1, -1, N, -1).reshape(B, R * N, 3).contiguous()
            coarse = nat.siren_forward(pts_c, rd, *(T(film[k]) for k in ("freq_geo", "phase_geo", "freq_app", "phase_app")))
            _, _, w_c, _ = native.composite(coarse.reshape(B * R, N, 22), z_c.reshape(B * R, N), noise_c.reshape(B * R, N), copts, want_wsum=False)
            depths.append(t64(native.resample(z_c.reshape(B * R, N), w_c, u).reshape(B, R, N)))
    sd64 = {k: t64(v) for k, v in sd.items()}
    args = tuple(t64(film[k]) for k in ("freq_geo", "phase_geo", "freq_app", "phase_app"))
    rows = []
    for z64 in depths:
        p = (o64.unsqueeze(2) + d64.unsqueeze(2) * z64.unsqueeze(-1)).reshape(B, R * N, 3)
        v = d64.unsqueeze(2).expand(-1, -1, N, -1).reshape(B, R * N, 3)
        rows.append(OG.siren_forward(sd64, spec, p, v, *args).reshape(B * R, N, 22))
    if hier:
        rgb, _, _ = OG.merge_composite(rows[1], rows[0], depths[1].reshape(B * R, N), depths[0].reshape(B * R, N), t64(noise_f.reshape(B * R, M)),
                                       noise_std=0.2, clamp_mode="relu")
    else:
        rgb, _, _ = OG.composite(rows[0], depths[0].reshape(B * R, N), t64(noise_f.reshape(B * R, M)), noise_std=0.2, clamp_mode="relu")
    ref_px = rgb.reshape(B, S_, S_, 21).permute(0, 3, 1, 2) * 2 - 1
    (ref_px * t64(w)).sum().backward()
    assert np.abs(N_(px) - ref_px.detach().numpy()).max() <= 1e-3
    e_y = abs(float(yaw.grad) - float(y64.grad)) / abs(float(y64.grad))
    e_p = abs(float(pitch.grad) - float(p64.grad)) / abs(float(p64.grad))
    print(f"[pose] generator pose gradient vs the fp64 chain [{'hierarchical' if hier else 'single pass'}, {'gaussian' if spread else 'fixed'} pose, "
          f"{precision}]: yaw {float(yaw.grad):+.5e} (rel. err {e_y:.2e}), pitch {float(pitch.grad):+.5e} (rel. err {e_p:.2e})")
    assert abs(float(y64.grad)) > 0 and abs(float(p64.grad)) > 0
    assert POSE_GRAD_BOUND is not None, "no measured bound recorded"
    assert e_y <= POSE_GRAD_BOUND[precision] and e_p <= POSE_GRAD_BOUND[precision], (e_y, e_p)


def test_generator_routes_that_cannot_deliver_pose_gradients_say_so(monkeypatch):
    """sparse_backward = True, the two-node (split) form and the AMP tiers raise NotImplementedError in the forward -- never a silent None
    for a pose that requires grad; sparse_backward = 'auto' takes the dense node and matches it bit for bit."""
    mod, spec, sd = _siren_module("texture", 32, 5, sigma_gain=150.0)
    gen = _double_generator(mod)
    B, S_, N = 2, 6, 8
    for hier in (True, False):
        kw = _pose_kw(S_, N, hier, True)
        px, _, yaw, pitch, film = _render_with_pose(gen, spec, B, kw)
        w = torch.randn(px.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
        (px * w).sum().backward()
        dense = (N_(px), float(yaw.grad), float(pitch.grad), {k: N_(v.grad) for k, v in film.items()})
        for p_ in mod.parameters():
            p_.grad = None
        monkeypatch.setattr(GA, "SPARSE_AUTO_MIN_SAMPLES", 0)             # (this render is tiny; without a pose 'auto' would now pick the sparse node)
        mod.sparse_backward = "auto"
        try:
            px, _, yaw, pitch, film = _render_with_pose(gen, spec, B, kw)
            (px * w).sum().backward()
            assert np.array_equal(N_(px), dense[0]) and float(yaw.grad) == dense[1] and float(pitch.grad) == dense[2]
            for k, v in film.items():
                assert np.array_equal(N_(v.grad), dense[3][k]), k
            mod.sparse_backward = True
            with pytest.raises(NotImplementedError, match="sparse_backward"):
                _render_with_pose(gen, spec, B, kw)
        finally:
            mod.sparse_backward = False
        mod.grad_precision = "amp"
        try:
            with pytest.raises(NotImplementedError, match="grad_precision"):
                _render_with_pose(gen, spec, B, kw)
        finally:
            mod.grad_precision = "f32"
    mod.split_backward = True
    try:
        with pytest.raises(NotImplementedError, match="split_backward"):
            _render_with_pose(gen, spec, B, _pose_kw(S_, N, True, True))
    finally:
        mod.split_backward = False


def test_single_latent_generator_and_part_forward_deliver_a_pose_gradient():
    """ImplicitGenerator3d and grad_points < R (part_forward) go through the same _render_grad: a finite, non-zero pose gradient"""
    mod, spec, sd = _siren_module("spatial", 32, 0, sigma_gain=120.0)
    gen = G.ImplicitGenerator3d(functools.partial(S.SPATIALSIRENBASELINE, hidden_dim=32), 8, 4)
    gen.siren = mod
    gen = gen.to(DEV)
    gen.device = torch.device(DEV); gen.siren.device = gen.device
    B, S_, N, H = 2, 5, 9, 32
    film = proc.film_params(spec, B, seed=4)
    film["freq_app"], film["phase_app"] = proc.normal("film.freq_app", (B, H), 0.4, 4), proc.normal("film.phase_app", (B, H), 0.4, 4)
    freq, phase = T(np.concatenate([film["freq_geo"], film["freq_app"]], -1)), T(np.concatenate([film["phase_geo"], film["phase_app"]], -1))
    for hier in (True, False):
        yaw = torch.tensor(YAW0, device=DEV, requires_grad=True)
        pitch = torch.tensor(PITCH0, device=DEV, requires_grad=True)
        torch.manual_seed(3)
        px, poses = gen.forward_with_frequencies(freq, phase, h_mean=yaw, v_mean=pitch, **_pose_kw(S_, N, hier, True))
        w = torch.randn(px.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
        (px * w).sum().backward()
        for g in (yaw.grad, pitch.grad):
            assert g is not None and bool(torch.isfinite(g)) and float(g.abs()) > 0
    mod2, spec2, _ = _siren_module("texture", 32, 5, sigma_gain=150.0)
    gen2 = _double_generator(mod2)
    z = torch.randn(B, 8, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    yaw = torch.tensor(YAW0, device=DEV, requires_grad=True)
    pitch = torch.tensor(PITCH0, device=DEV, requires_grad=True)
    torch.manual_seed(3)
    px, poses = gen2(z, z, h_mean=yaw, v_mean=pitch, grad_points=20, **_pose_kw(8, 8, True, False))
    assert poses.requires_grad
    w = torch.randn(px.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    (px * w).sum().backward()
    for g in (yaw.grad, pitch.grad):
        assert g is not None and bool(torch.isfinite(g)) and float(g.abs()) > 0


# ------------------------------------------------------------------------------------------------------------------------------------
# 5. callers.inverse_render(optimize_pose=True) and the command line
# ------------------------------------------------------------------------------------------------------------------------------------
class _FixedDraws(VR.TorchDraws):      # no jitter, no noise: the render is a function of the FiLM parameters and the pose only
    def rand(self, shape, device):
        return torch.full(shape, 0.5, device=device)

    def randn(self, shape, device):
        return torch.zeros(shape, device=device)


def test_inverse_render_optimizes_the_pose():
    """The tiny generator at 16 x 16; target = its own render at yaw pi/2 + 0.15 with the true FiLM state (zero offsets are the optimum).
    optimize_pose=True, 20 iterations: the yaw moves, the loss falls, and the first iteration's yaw gradient has the sign the fp64 oracle
    gives (fp64 torch rays -> oracle SIREN -> composite -> loss, differentiated in the yaw).
    optimize_pose=False: offsets and losses bit-identical to the call on the previous signature, the yaw untouched."""
    from fenerf_amd import callers
    torch.manual_seed(7)
    mod, spec, sd = _siren_module("texture", 32, 5, sigma_gain=150.0)
    gen = _double_generator(mod).eval()
    for p in gen.parameters():
        p.requires_grad_(False)
    gen.draws = _FixedDraws()
    hv = math.pi / 2
    opts = dict(img_size=16, fov=12, ray_start=0.88, ray_end=1.12, num_steps=12, h_stddev=0, v_stddev=0, h_mean=torch.tensor(hv, device=DEV),
                v_mean=torch.tensor(hv, device=DEV), hierarchical_sample=False, sample_dist=None, clamp_mode="relu", nerf_noise=0, last_back=False)
    with torch.no_grad():       # the FiLM state inverse_render starts from with init_psi = 0: the mean over its 10,000 latents (zero draws: one latent)
        fg, pg = gen.siren.geo_mapping_network(torch.zeros(1, 8, device=DEV))
        fa, pa = gen.siren.app_mapping_network(torch.zeros(1, 8, device=DEV))
        render = lambda yaw: gen.forward_with_frequencies(fg, fa, pg, pa, **dict(opts, h_mean=yaw))[0]
        target = render(hv + 0.15)
    # d loss / d yaw at the start from the fp64 oracle: fp64 torch rays -> points -> oracle SIREN -> composite -> the two MSE terms
    from oracle import fenerf_oracle_grad as OG
    t64 = lambda a: torch.as_tensor(N_(a) if torch.is_tensor(a) else np.asarray(a), dtype=torch.float64)
    S_, N, R = 16, 12, 256
    y64 = torch.tensor(float(np.float32(hv)), dtype=torch.float64, requires_grad=True)
    ang = torch.ones((1, 1), dtype=torch.float64)
    o64, d64, _, _ = VR.rays_from_angles(ang * y64, ang * float(np.float32(hv)), (S_, S_), 12, "cpu")
    z64 = t64(VR.sample_rays(1, N, gen.device, 12, (S_, S_), 0.88, 1.12, 0, 0, hv, hv, None, draws=gen.draws)[2].reshape(1, R, N))
    pts = (o64.unsqueeze(2) + d64.unsqueeze(2) * z64.unsqueeze(-1)).reshape(1, R * N, 3)
    rows = OG.siren_forward({k: t64(v) for k, v in sd.items()}, spec, pts, d64.unsqueeze(2).expand(-1, -1, N, -1).reshape(1, R * N, 3),
                            t64(fg), t64(pg), t64(fa), t64(pa))
    rgb, _, _ = OG.composite(rows.reshape(R, N, 22), z64.reshape(R, N), None, noise_std=0.0, clamp_mode="relu")
    frame = rgb.reshape(1, S_, S_, 21).permute(0, 3, 1, 2) * 2 - 1
    (((frame[:, :-3] - t64(target[:, :-3])) ** 2).mean() + ((frame[:, -3:] - t64(target[:, -3:])) ** 2).mean()).backward()
    slope = float(y64.grad)
    assert slope != 0
    first = {}
    res = callers.inverse_render(gen, target[:, -3:], target[:, :-3], opts, n_iterations=20, z_dim=8, latent_noise=0.0, n_mean_latents=4,
                                 optimize_pose=True,
                                 on_step=lambda i, loss, meta: first.setdefault("yaw", float(meta["yaw"])) if i == 0 else None)
    assert set(res) >= {"yaw", "pitch", "losses"} and isinstance(res["yaw"], float) and isinstance(res["pitch"], float)
    print(f"[pose] inverse_render(optimize_pose=True), 20 iterations: yaw {hv:.4f} -> {res['yaw']:.4f} (target {hv + 0.15:.4f}), pitch -> {res['pitch']:.4f}, "
          f"loss {res['losses'][0]:.4e} -> {res['losses'][-1]:.4e}; d loss / d yaw at the start (fp64 oracle) {slope:+.3e}")
    assert res["yaw"] != hv and res["losses"][-1] < res["losses"][0]
    assert (first["yaw"] - float(np.float32(hv))) * slope < 0, "Adam's first step moves the yaw against the gradient: its sign is the oracle's"
    assert float(opts["h_mean"]) == np.float32(hv), "the caller's options are not modified"
    # optimize_pose=False: today's values, bit for bit
    a = callers.inverse_render(gen, target[:, -3:], target[:, :-3], opts, n_iterations=5, z_dim=8, latent_noise=0.0, n_mean_latents=4)
    b = callers.inverse_render(gen, target[:, -3:], target[:, :-3], opts, n_iterations=5, z_dim=8, latent_noise=0.0, n_mean_latents=4, optimize_pose=False)
    assert a["losses"] == b["losses"] and a["yaw"] == b["yaw"] == float(np.float32(hv)) and a["pitch"] == float(np.float32(hv))
    for k in a:
        if "offset" in k:
            assert torch.equal(a[k], b[k]), k
    # ... and the yaw passed as a plain number gives the same losses as the tensor the options carry
    c = callers.inverse_render(gen, target[:, -3:], target[:, :-3], dict(opts, h_mean=float(np.float32(hv)), v_mean=float(np.float32(hv))), n_iterations=5,
                               z_dim=8, latent_noise=0.0, n_mean_latents=4)
    assert c["losses"] == a["losses"]


def test_inverse_render_cli_optimize_pose(tmp_path):
    """tools/inverse_render.py --optimize_pose --lr_pose parses and runs for 2 iterations; the checkpoint gains yaw / pitch"""
    import subprocess
    import sys
    from PIL import Image
    from conftest import ROOT
    from test_gpu_parity import _tiny_checkpoint_dir
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import inverse_render
        o = inverse_render.build_parser().parse_args(["n", "g.pth", "--optimize_pose", "--lr_pose", "0.05"])
        assert o.optimize_pose is True and o.lr_pose == 0.05
        o = inverse_render.build_parser().parse_args(["n", "g.pth"])
        assert o.optimize_pose is False and o.lr_pose is None
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    ckpt = _tiny_checkpoint_dir(tmp_path)
    rng = np.random.default_rng(0)
    Image.fromarray(rng.integers(0, 255, (40, 32, 3), dtype=np.uint8)).save(str(tmp_path / "face.jpg"))
    lab = np.zeros((40, 32), np.uint8); lab[8:30, 6:26] = 1; lab[12:16, 10:14] = 4
    Image.fromarray(lab, "L").save(str(tmp_path / "face.png"))
    out = str(tmp_path / "inv")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "inverse_render.py"), "t", ckpt, "--image_path", str(tmp_path / "face.jpg"), "--seg_path",
           str(tmp_path / "face.png"), "--save_dir", out, "--image_size", "8", "--iteration", "2", "--lambda_seg", "1", "--lambda_img", "1", "--no_center_crop", "--preview_size", "8",
           "--preview_steps", "6", "--optimize_pose", "--lr_pose", "0.05"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    meta = torch.load(os.path.join(out, "freq_phase_offset_t.pth"), weights_only=False)
    assert isinstance(meta["yaw"], float) and isinstance(meta["pitch"], float) and meta["yaw"] != float(np.float32(math.pi / 2))
    assert "yaw" in r.stdout
