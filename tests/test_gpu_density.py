"""The geometry route (include/fenerf.h "The geometry route"): labels and sigma without the colour branch -- fenerf_siren_density,
fenerf_siren_density_rays, fenerf_render_density and what the Python package builds on them -- against the code that exists without it:
the dense siren_forward / siren_forward_rays / render and staged_forward.  Every comparison is bit for bit, NaNs in the same places; there
are no tolerances and no excluded elements."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest
import torch

from fenerf_amd import _lib, callers, native, procedural as proc
from fenerf_amd.generators import generators as G
from fenerf_amd.generators import volumetric_rendering as VR
from fenerf_amd.siren import siren as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POINT_COUNTS = (1, 15, 16, 17, 127, 129, 245, 2051)     # a phantom-lane tile, one tile, a tile edge, a partial oct, an oct edge, many workgroups
SENTINEL = -12345.678


def T(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float32), device=DEV)


def _same(x, y, what):
    assert x.shape == y.shape, (what, tuple(x.shape), tuple(y.shape))
    assert torch.equal(torch.isnan(x), torch.isnan(y)), (what, "NaNs sit in the same places")
    assert torch.equal(torch.nan_to_num(x, nan=-7.0), torch.nan_to_num(y, nan=-7.0)), (what, float((x - y).abs().nan_to_num().max()))


@functools.lru_cache(maxsize=None)
def _state(kind, H, grid):
    spec = proc.model_spec(kind, hidden_dim=H, grid_size=grid, z_dim=8)
    return spec, proc.make_state_dict(spec, seed=6, sigma_gain=60.0, with_mapping=False)


@functools.lru_cache(maxsize=None)
def _model(kind, H, grid, precision="f16x3"):
    spec, sd = _state(kind, H, grid)
    return native.NativeModel(sd, spec, DEV, precision)


def _film(spec, B, seed=3):
    film = proc.film_params(spec, B, seed=seed)
    if spec["kind"] == "spatial":       # single latent: the colour layer's block is the ninth slice of the same mapping output
        H = spec["hidden_dim"]
        film["freq_app"] = proc.normal("film.freq_app", (B, H), 0.4, seed)
        film["phase_app"] = proc.normal("film.phase_app", (B, H), 0.4, seed)
    return tuple(T(film[k]) for k in ("freq_geo", "phase_geo", "freq_app", "phase_app"))


def _points(B, P, seed=1):
    rng = np.random.default_rng(seed + 100 * P + B)
    pts = rng.uniform(-0.125, 0.125, (B, P, 3)).astype(np.float32)       # some points leave the grid box
    dirs = rng.normal(size=(B, P, 3)).astype(np.float32)
    dirs /= np.linalg.norm(dirs, axis=-1, keepdims=True)
    return T(pts), T(dirs)


def _geo(full, nat):
    """[labels | sigma] of full rows"""
    n = nat.n_labels()
    return torch.cat([full[..., :n], full[..., -1:]], dim=-1) if n else full[..., -1]


def _check_points(nat, spec, B, P, what):
    fg, pg, fa, pa = _film(spec, B)
    pts, dirs = _points(B, P)
    full = nat.siren_forward(pts, dirs, fg, pg, fa, pa)
    rows = nat.siren_density(pts, fg, pg, labels=True)
    sigma = nat.siren_density(pts, fg, pg, labels=False)
    torch.cuda.synchronize()
    n = nat.n_labels()
    assert tuple(sigma.shape) == (B, P) and tuple(rows.shape) == ((B, P, n + 1) if n else (B, P))
    _same(rows, _geo(full, nat), what + " labels|sigma")
    _same(sigma, full[..., -1], what + " sigma")
    _same(sigma, rows[..., -1] if n else rows, what + " sigma alone = last column of the compact rows")


MODELS = {"h32-grid": ("texture", 32, 8), "h96-grid": ("texture", 96, 8), "h256-grid": ("texture", 256, 8), "h32-nogrid": ("baseline", 32, 0),
          "h96-nogrid": ("baseline", 96, 0), "h256-nogrid": ("baseline", 256, 0), "h40-padded-grid": ("texture", 40, 8)}


@pytest.mark.parametrize("model", list(MODELS))
def test_point_query_equals_the_dense_forward(model):
    kind, H, grid = MODELS[model]
    spec, _ = _state(kind, H, grid)
    nat = _model(kind, H, grid)
    assert nat.supports_density() and nat.n_labels() == 18
    if model == "h40-padded-grid":
        assert nat.padded and nat.spec["hidden_dim"] == native.padded_hidden_dim(40)
    for B in (1, 2):                    # B = 2 with P = 245 (no multiple of 32): a launch per image
        for P in POINT_COUNTS:
            _check_points(nat, spec, B, P, f"{model} B{B} P{P}")


def test_point_query_of_a_model_without_labels():
    spec, _ = _state("spatial", 32, 0)
    nat = _model("spatial", 32, 0)
    assert nat.n_labels() == 0 and nat.supports_density()
    for B, P in ((1, 17), (2, 245), (1, 2051)):
        _check_points(nat, spec, B, P, f"spatial B{B} P{P}")


def test_point_query_at_forward_mode_f16x3c2():
    """that mode's sigma and labels are the default's bits by construction: the query serves it, against the mode's own full forward"""
    spec, _ = _state("texture", 32, 8)
    nat = _model("texture", 32, 8, "f16x3c2")
    assert nat.supports_density()
    for B, P in ((1, 129), (2, 245)):
        _check_points(nat, spec, B, P, f"f16x3c2 B{B} P{P}")
    fg, pg, fa, pa = _film(spec, 1)
    pts, _ = _points(1, 129)
    _same(nat.siren_density(pts, fg, pg), _model("texture", 32, 8).siren_density(pts, fg, pg), "f16x3c2 = default")


def _rays(spec, B, S_, N, seed=0):
    torch.manual_seed(12 + seed)
    o, d, z, _, _ = VR.sample_rays(B, N, DEV, 12, (S_, S_), 0.88, 1.12, 0.3, 0.155, np.pi / 2, np.pi / 2, "gaussian")
    u = torch.rand((B * S_ * S_, N), device=DEV)
    return dict(o=o, d=d, z=z, u=u, film=_film(spec, B, seed=seed))


@pytest.mark.parametrize("shape", [(2, 8, 6), (1, 7, 5)], ids=["b2-8x8x6", "b1-7x7x5"])
@pytest.mark.parametrize("model", ["h32-grid", "h96-nogrid"])
def test_ray_query_equals_the_dense_forward(model, shape):
    kind, H, grid = MODELS[model]
    B, S_, N = shape
    spec, _ = _state(kind, H, grid)
    nat = _model(kind, H, grid)
    a = _rays(spec, B, S_, N)
    full = nat.siren_forward_rays(a["o"], a["d"], a["z"], *a["film"])
    rows = nat.siren_density_rays(a["o"], a["d"], a["z"], a["film"][0], a["film"][1])
    sigma = nat.siren_density_rays(a["o"], a["d"], a["z"], a["film"][0], a["film"][1], labels=False)
    assert tuple(rows.shape) == (B, S_ * S_, N, 19) and tuple(sigma.shape) == (B, S_ * S_, N)
    _same(rows, _geo(full, nat), "rays labels|sigma")
    _same(sigma, full[..., -1], "rays sigma")


def test_independent_of_the_colour_inputs():
    """NaN appearance parameters and infinite view directions in the dense call change neither its sigma nor its labels; the density call is
    never given them"""
    spec, _ = _state("texture", 32, 8)
    nat = _model("texture", 32, 8)
    fg, pg, fa, pa = _film(spec, 2)
    pts, dirs = _points(2, 245)
    full = nat.siren_forward(pts, torch.full_like(dirs, float("inf")), fg, pg, torch.full_like(fa, float("nan")), torch.full_like(pa, float("nan")))
    assert torch.isnan(full[..., -4:-1]).all()          # the dense call's rgb is NaN there: not compared
    _same(nat.siren_density(pts, fg, pg), _geo(full, nat), "colour inputs")
    _same(nat.siren_density(pts, fg, pg), _geo(nat.siren_forward(pts, dirs, fg, pg, fa, pa), nat), "clean colour inputs")


def test_nonfinite_coordinates_stay_in_their_rows():
    spec, _ = _state("texture", 32, 8)
    nat = _model("texture", 32, 8)
    fg, pg, fa, pa = _film(spec, 1)
    pts, dirs = _points(1, 129)
    clean = nat.siren_density(pts, fg, pg)
    bad = pts.clone()
    bad[0, 5, 0] = float("nan")           # a lane of tile 0
    bad[0, 40, 1] = float("inf")          # a lane of tile 2
    got = nat.siren_density(bad, fg, pg)
    _same(got, _geo(nat.siren_forward(bad, dirs, fg, pg, fa, pa), nat), "non-finite coordinates")
    keep = torch.ones(129, dtype=torch.bool, device=DEV)
    keep[[5, 40]] = False
    _same(got[0, keep], clean[0, keep], "neighbouring rows")
    assert not torch.isfinite(got[0, 5]).all() and not torch.isfinite(got[0, 40]).all()


@pytest.mark.parametrize("labels", [True, False], ids=["labels", "sigma"])
def test_red_zone(labels):
    """the buffer over-allocated by a tile's worth of rows on each side: the margins keep their sentinel, every element between is written"""
    spec, _ = _state("texture", 32, 8)
    nat = _model("texture", 32, 8)
    row = 19 if labels else 1
    for B in (1, 2):
        fg, pg, _, _ = _film(spec, B)
        for P in POINT_COUNTS:
            pts, _ = _points(B, P)
            want = nat.siren_density(pts, fg, pg, labels=labels)
            margin, n = 16 * row, B * P * row
            buf = torch.full((margin + n + margin,), SENTINEL, dtype=torch.float32, device=DEV)
            out = buf[margin:margin + n].view((B, P, row) if labels else (B, P))
            nat.siren_density(pts, fg, pg, labels=labels, out=out)
            torch.cuda.synchronize()
            assert bool((buf[:margin] == SENTINEL).all()) and bool((buf[margin + n:] == SENTINEL).all()), (B, P, "margins")
            _same(out, want, f"B{B} P{P} in-range elements")
            assert not bool((out == SENTINEL).any()), (B, P, "every in-range element written")


# ---- render_density against render
RENDER_SHAPES = {
    "h32-b2-8x8x6": ("texture", 32, 8, 2, 8, 6, True),
    "h32-b1-7x7x5": ("texture", 32, 8, 1, 7, 5, True),
    "h256-b1-8x8x12": ("texture", 256, 8, 1, 8, 12, True),
    "h32-b1-8x8x3-smallest-hierarchical": ("texture", 32, 8, 1, 8, 3, True),
    "h32-b2-8x8x6-single-pass": ("texture", 32, 8, 2, 8, 6, False),
}
OPTS = {
    "relu-seg-padding-black": dict(clamp_mode="relu", fill_mode="seg_padding_background", fill_color="black"),
    "softplus": dict(clamp_mode="softplus"),
    "noise": dict(clamp_mode="relu", noise_std=0.5),
    "last-back": dict(clamp_mode="relu", last_back=True),
    "white-back": dict(clamp_mode="relu", white_back=True),
}


def _opts(name):
    return _lib.composite_opts(**OPTS[name])


def _check_render(nat, a, opts, hier, what, noise=False, split_force=False):
    B, R, N = a["z"].shape
    M = 2 * N if hier else N
    nc = nf = None
    if noise:
        g = torch.Generator(device=DEV).manual_seed(3)
        nc, nf = torch.randn((B, R, N), device=DEV, generator=g), torch.randn((B, R, M), device=DEV, generator=g)
    n_lab = nat.n_labels()
    dens = nat.render_density(a["o"], a["d"], a["z"], a["u"] if hier else None, nc, nf, a["film"][0], a["film"][1], opts, hierarchical=hier, labels=True,
                              want_weights=True, want_wsum=True)
    bare = nat.render_density(a["o"], a["d"], a["z"], a["u"] if hier else None, nc, nf, a["film"][0], a["film"][1], opts, hierarchical=hier, labels=False,
                              want_weights=True, want_wsum=True)
    assert bare[0] is None
    for mode in ["off"] + (["force"] if split_force and hier else []):
        with native.render_split(mode), native.render_fusion("off"):
            full = nat.render(a["o"], a["d"], a["z"], a["u"] if hier else None, nc, nf, *a["film"], opts, hierarchical=hier, want_weights=True, want_wsum=True)
            torch.cuda.synchronize()
        if n_lab:
            _same(dens[0], full[0][..., :full[0].shape[-1] - 3].contiguous(), f"{what} split {mode}: label channels")
        else:
            assert dens[0] is None
        for name, i in (("depth", 1), ("weights", 2), ("weights_sum", 3)):
            _same(dens[i], full[i], f"{what} split {mode}: {name}")
            _same(bare[i], full[i], f"{what} split {mode}: {name} of the render without labels")


@pytest.mark.parametrize("shape", list(RENDER_SHAPES))
def test_render_density_equals_the_render(shape):
    kind, H, grid, B, S_, N, hier = RENDER_SHAPES[shape]
    spec, _ = _state(kind, H, grid)
    nat = _model(kind, H, grid)
    a = _rays(spec, B, S_, N)
    _check_render(nat, a, _opts("relu-seg-padding-black"), hier, shape, split_force=True)
    _check_render(nat, a, _opts("softplus"), hier, shape + " softplus")


@pytest.mark.parametrize("case", list(OPTS))
def test_render_density_option_cases(case):
    spec, _ = _state("texture", 32, 8)
    nat = _model("texture", 32, 8)
    a = _rays(spec, 2, 8, 6, seed=1)
    _check_render(nat, a, _opts(case), True, case, noise=case == "noise", split_force=case in ("relu-seg-padding-black", "white-back"))


def test_render_density_eval_white_back_and_no_labels():
    """eval_white_back needs a model of three colour channels: no labels, a depth and weights render"""
    spec, _ = _state("spatial", 32, 0)
    nat = _model("spatial", 32, 0)
    a = _rays(spec, 2, 8, 6)
    for kw in (dict(clamp_mode="relu", fill_mode="eval_white_back"), dict(clamp_mode="relu")):
        _check_render(nat, a, _lib.composite_opts(**kw), True, "spatial " + str(kw), split_force=True)


def test_phase_timers_count_the_density_launches():
    spec, _ = _state("texture", 32, 8)
    nat = _model("texture", 32, 8)
    a = _rays(spec, 1, 8, 6)
    with native.phase_timing() as t:
        nat.render_density(a["o"], a["d"], a["z"], a["u"], None, None, a["film"][0], a["film"][1], _opts("softplus"))
        torch.cuda.synchronize()
    assert t.calls.get("siren_density") == 2 and t.calls.get("siren_forward") == 2, t.calls


# ---- refusals
def test_refusals_launch_nothing():
    spec, sd = _state("texture", 32, 8)
    fg, pg, fa, pa = _film(spec, 1)
    pts, _ = _points(1, 33)
    for precision in ("f32", "f16x2"):
        nat = _model("texture", 32, 8, precision)
        assert not nat.supports_density()
        out = torch.full((1, 33, 19), SENTINEL, device=DEV)
        with pytest.raises(_lib.FenerfError) as e:
            nat.siren_density(pts, fg, pg, out=out)
        assert e.value.code == _lib.E_UNSUPPORTED and len(str(e.value)) > 40, str(e.value)
        a = _rays(spec, 1, 8, 6)
        with pytest.raises(_lib.FenerfError) as e:
            nat.siren_density_rays(a["o"], a["d"], a["z"], fg, pg)
        assert e.value.code == _lib.E_UNSUPPORTED
        with pytest.raises(_lib.FenerfError) as e:
            nat.render_density(a["o"], a["d"], a["z"], a["u"], None, None, fg, pg, _opts("softplus"))
        assert e.value.code == _lib.E_UNSUPPORTED
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all())
    nat = _model("texture", 32, 8)
    l = _lib.lib()
    P_ = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    out = torch.full((1, 33, 19), SENTINEL, device=DEV)
    ws = torch.empty(l.fenerf_film_workspace_bytes(nat._h, 1), dtype=torch.uint8, device=DEV)
    ok = (nat._h, 1, 33, P_(pts), P_(fg), P_(pg), 1, P_(out), P_(ws), None)
    for i, v in ((0, None), (3, None), (4, None), (5, None), (7, None), (8, None), (1, 0), (1, -1), (2, -5)):
        args = list(ok)
        args[i] = v
        assert l.fenerf_siren_density(*args) == _lib.E_INVALID, i
        assert l.fenerf_last_error()
    assert l.fenerf_siren_density(*(list(ok[:2]) + [0] + list(ok[3:]))) == _lib.OK        # P = 0: nothing launched
    a = _rays(spec, 1, 8, 6)
    rows = torch.full((1, 64, 6, 19), SENTINEL, device=DEV)
    okr = (nat._h, 1, 64, 6, P_(a["o"]), P_(a["d"]), P_(a["z"]), P_(fg), P_(pg), 1, P_(rows), P_(ws), None)
    for i, v in ((4, None), (5, None), (6, None), (7, None), (10, None), (11, None), (2, -1), (3, 0)):
        args = list(okr)
        args[i] = v
        assert l.fenerf_siren_density_rays(*args) == _lib.E_INVALID, i
    opts = _opts("softplus")
    need = l.fenerf_render_density_workspace_bytes(nat._h, 1, 64, 6, 1, 1)
    assert need > 0 and l.fenerf_render_density_workspace_bytes(nat._h, 1, 64, 6, 1, 0) < need
    rws = torch.empty(need, dtype=torch.uint8, device=DEV)
    lab, dep = torch.full((1, 64, 18), SENTINEL, device=DEV), torch.full((1, 64), SENTINEL, device=DEV)
    okd = [nat._h, 1, 64, 6, 1, P_(a["o"]), P_(a["d"]), P_(a["z"]), P_(a["u"]), None, None, P_(fg), P_(pg), C.byref(opts), 1, P_(lab), P_(dep), None, None,
           P_(rws), C.c_size_t(need), None]
    for i, v in ((0, None), (5, None), (6, None), (7, None), (8, None), (11, None), (12, None), (13, None), (15, None), (19, None),
                 (20, C.c_size_t(need - 1)), (1, -1), (2, -1), (3, 0), (3, 2), (3, 513)):
        args = list(okd)
        args[i] = v
        assert l.fenerf_render_density(*args) == _lib.E_INVALID, i
    assert l.fenerf_render_density(*(okd[:2] + [0] + okd[3:])) == _lib.OK                  # B * R = 0: nothing launched
    torch.cuda.synchronize()
    for t in (out, rows, lab, dep):
        assert bool((t == SENTINEL).all())
    assert l.fenerf_render_density(*okd) == _lib.OK
    torch.cuda.synchronize()
    assert not bool((lab == SENTINEL).any()) and not bool((dep == SENTINEL).any())


# ---- the Python surface
def _siren_module(kind, H, grid, precision="f16x3", sigma_gain=150.0):
    spec = proc.model_spec(kind, hidden_dim=H, grid_size=grid, z_dim=8)
    sd = proc.make_state_dict(spec, seed=4, sigma_gain=sigma_gain, with_mapping=False)
    cls = {"texture": S.TextureEmbeddingPiGAN128SEMANTICDISENTANGLE, "baseline": S.SIRENBASELINESEMANTICDISENTANGLE}[kind]
    torch.manual_seed(0)                  # the mapping networks of the module are torch-initialised
    mod = cls(hidden_dim=H, z_geo_dim=8, z_app_dim=8, output_dim=22)
    tsd = {k: torch.from_numpy(v) for k, v in sd.items()}
    if "spatial_embeddings" in tsd:
        mod.spatial_embeddings = torch.nn.Parameter(tsd["spatial_embeddings"].clone())
    mod.load_state_dict(tsd, strict=False)
    mod.precision = precision
    mod = mod.to(DEV)
    mod.device = torch.device(DEV)
    return mod, spec


def _generator(softmax_label=False, precision="f16x3"):
    mod, spec = _siren_module("texture", 32, 6, precision)
    gen = G.DoubleImplicitGenerator3d(functools.partial(S.TextureEmbeddingPiGAN128SEMANTICDISENTANGLE, hidden_dim=32), 8, 8, 22, softmax_label=softmax_label)
    gen.siren = mod
    gen = gen.to(DEV).eval()
    gen.device = torch.device(DEV)
    gen.siren.device = gen.device
    return gen


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_siren_geometry(precision):
    mod, _ = _siren_module("texture", 32, 6, precision)
    pts, dirs = _points(2, 96)
    torch.manual_seed(1)
    z_geo, z_app = torch.randn(2, 8, device=DEV), torch.randn(2, 8, device=DEV)
    with torch.no_grad():
        full = mod(pts, z_geo, z_app, dirs)
        got = mod.geometry(pts, z_geo)
    assert mod.native(DEV).supports_density() == (precision == "f16x3")
    assert got.grad_fn is None
    _same(got, torch.cat([full[..., :-4], full[..., -1:]], -1), "siren.geometry without grad")
    z_req = z_geo.clone().requires_grad_(True)
    out = mod.geometry(pts, z_req)
    assert out.grad_fn is not None and tuple(out.shape) == (2, 96, 19)
    out[..., -1].sum().backward()
    assert z_req.grad is not None and bool(torch.isfinite(z_req.grad).all()) and float(z_req.grad.abs().max()) > 0


def _rng_get():
    return torch.get_rng_state(), torch.cuda.get_rng_state(DEV)


def _rng_set(state):
    torch.set_rng_state(state[0])
    torch.cuda.set_rng_state(state[1], DEV)


def _rng_equal(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


STAGED = dict(img_size=8, fov=12, ray_start=0.88, ray_end=1.12, num_steps=6, h_stddev=0.3, v_stddev=0.155, h_mean=math.pi / 2, v_mean=math.pi / 2,
              hierarchical_sample=True, sample_dist="gaussian", clamp_mode="relu", nerf_noise=0.1, last_back=False, psi=0.7)


@pytest.mark.parametrize("fill", ["eval_seg_padding_background", None], ids=["padding-background", "no-fill"])
@pytest.mark.parametrize("softmax_label", [False, True], ids=["logits", "softmax"])
def test_staged_geometry_equals_staged_forward(softmax_label, fill):
    gen = _generator(softmax_label)
    kw = dict(STAGED, fill_mode=fill, fill_color="black")
    torch.manual_seed(5)
    z_geo, z_app = torch.randn(1, 8, device=DEV), torch.randn(1, 8, device=DEV)
    state = _rng_get()
    img, depth = gen.staged_forward(z_geo, z_app, **kw)
    after = _rng_get()
    _rng_set(state)
    lab, depth2 = gen.staged_geometry(z_geo, None, **kw)
    assert _rng_equal(_rng_get(), after)            # the generator is consumed alike
    assert lab.device.type == "cpu" and tuple(lab.shape) == (1, img.shape[1] - 3, 8, 8)
    _same(lab, img[:, :-3], "staged_geometry labels")
    _same(depth2, depth, "staged_geometry depth")
    # the *_with_frequencies twin
    fg, pg, fa, pa = _film(proc.model_spec("texture", hidden_dim=32, grid_size=6, z_dim=8), 1, seed=4)
    kw.pop("psi")
    _rng_set(state)
    img, depth, _ = gen.staged_forward_with_frequencies(fg, fa, pg, pa, **kw)
    _rng_set(state)
    lab, depth2 = gen.staged_geometry_with_frequencies(fg, None, pg, None, **kw)
    _same(lab, img[:, :-3], "staged_geometry_with_frequencies labels")
    _same(depth2, depth, "staged_geometry_with_frequencies depth")


def test_staged_geometry_falls_back_on_an_f32_model():
    gen = _generator(precision="f32")
    kw = dict(STAGED, fill_mode="eval_seg_padding_background", fill_color="black")
    torch.manual_seed(5)
    z_geo, z_app = torch.randn(1, 8, device=DEV), torch.randn(1, 8, device=DEV)
    state = _rng_get()
    img, depth = gen.staged_forward(z_geo, z_app, **kw)
    _rng_set(state)
    lab, depth2 = gen.staged_geometry(z_geo, z_app, **kw)
    _same(lab, img[:, :-3], "f32 fallback labels")
    _same(depth2, depth, "f32 fallback depth")


def test_staged_geometry_of_the_single_latent_generator():
    """no label channels: the depth map of staged_forward, through the density route"""
    torch.manual_seed(0)
    gen = G.ImplicitGenerator3d(functools.partial(S.SPATIALSIRENBASELINE, hidden_dim=32), 8, 4).to(DEV).eval()
    gen.device = torch.device(DEV)
    gen.siren.device = gen.device
    assert gen.siren.native(DEV).supports_density() and gen.siren.native(DEV).n_labels() == 0
    kw = dict(STAGED, fill_mode=None, fill_color="black")
    torch.manual_seed(5)
    z = torch.randn(1, 8, device=DEV)
    state = _rng_get()
    _, depth, _ = gen.staged_forward(z, **kw)
    after = _rng_get()
    _rng_set(state)
    lab, depth2 = gen.staged_geometry(z, **kw)
    assert _rng_equal(_rng_get(), after) and tuple(lab.shape) == (1, 0, 8, 8)
    _same(depth2, depth, "single-latent depth")


def test_callers_take_the_density_route_with_the_same_bytes(monkeypatch):
    gen = _generator()
    torch.manual_seed(3)
    z = torch.randn(1, 8, device=DEV)

    def run():
        torch.manual_seed(7)
        vol, lab = callers.sample_generator(gen, z, cube_length=0.3, voxel_resolution=12, return_labels=True)
        torch.manual_seed(7)
        assert np.array_equal(callers.sample_generator(gen, z, cube_length=0.3, voxel_resolution=12).view(np.uint32), vol.view(np.uint32))
        fg, pg, fa, pa = _film(proc.model_spec("texture", hidden_dim=32, grid_size=6, z_dim=8), 1, seed=4)
        meta = dict(truncated_frequencies_geo=fg, truncated_phase_shifts_geo=pg, truncated_frequencies_app=fa, truncated_phase_shifts_app=pa)
        vol2 = callers.sample_generator_wth_frequencies_phase_shifts(gen, meta, cube_length=0.3, voxel_resolution=12)
        mesh = callers.extract_mesh(gen, None, film=meta, voxel_resolution=12, cube_length=0.3, iso=float(np.median(vol2)), attributes=("label",))
        return vol, lab, vol2, mesh

    calls = []
    real = native.NativeModel.siren_density
    monkeypatch.setattr(native.NativeModel, "siren_density", lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    new = run()
    assert len(calls) == 4          # the three lattice passes + the labelled one: the density route ran
    monkeypatch.setattr(native.NativeModel, "supports_density", lambda self: False)
    old = run()
    assert len(calls) == 4
    assert new[0].shape == (12, 12, 12) and new[1].shape == (12, 12, 12) and new[1].dtype == np.uint8
    for a, b in zip(new[:3], old[:3]):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
    assert len(new[3]["vertices"]) > 0
    for k in ("vertices", "faces", "label"):
        assert np.array_equal(new[3][k], old[3][k]), k
    # the label volume = the argmax of the full rows
    torch.manual_seed(7)
    samples, _, _ = callers.create_samples(12, (0, 0, 0), 0.3, device=z.device)
    avg = gen.generate_avg_frequencies()
    with torch.no_grad():
        raw = gen.siren.geo_mapping_network(z) + gen.siren.app_mapping_network(z)
        fg, pg, fa, pa = (avg[i] + 0.5 * (raw[i] - avg[i]) for i in range(4))
        rows = gen.siren.native(torch.device(DEV)).siren_forward(samples, None, fg, pg, fa, pa)
    assert np.array_equal(new[1].reshape(-1), torch.argmax(rows[0, :, :-4], dim=-1).cpu().numpy().astype(np.uint8))


def test_render_multiview_labels_only():
    gen = _generator()
    cur = {0: dict(batch_size=1, num_steps=6, img_size=8), "fov": 12, "ray_start": 0.88, "ray_end": 1.12, "h_stddev": 0.3, "v_stddev": 0.155,
           "h_mean": math.pi / 2, "v_mean": math.pi / 2, "sample_dist": "gaussian", "clamp_mode": "relu", "hierarchical_sample": True,
           "fill_mode": "eval_seg_padding_background", "nerf_noise": 0, "last_back": False, "white_back": False, "psi": 0.7}
    _, seg = callers.render_multiview(gen, cur, 2, torch.device(DEV), image_size=8, ray_step_multiplier=1, z_dim=8)
    seg2, depth = callers.render_multiview(gen, cur, 2, torch.device(DEV), image_size=8, ray_step_multiplier=1, z_dim=8, labels_only=True)
    assert tuple(depth.shape) == (5, 8, 8)
    _same(seg2, seg, "semantic row")
