"""The split coarse pass of the hierarchical render (fenerf_set_render_split): a density launch that lists the samples with sigma > 0 and
a colour launch over the listed samples only must give the dense route's rgb, depth, weights and weights_sum bit for bit, NaNs in the
same places -- per-image lists, partial tiles and octs, the capacity edge, empty lists, stale workspaces, non-finite colour inputs."""
import functools

import numpy as np
import pytest
import torch

from fenerf_amd import _lib, native, procedural as proc
from fenerf_amd.generators import volumetric_rendering as VR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("rgb", "depth", "weights", "weights_sum")

# id: (kind, hidden_dim, grid_size, B, S, N)
SHAPES = {
    "h32-grid8-b2-8x8x6": ("texture", 32, 8, 2, 8, 6),       # per-image lists; tiles that straddle rays (384 points per image)
    "h32-grid8-b1-7x7x5": ("texture", 32, 8, 1, 7, 5),       # phantom lanes; a partial last oct (245 points)
    "h256-grid8-b1-8x8x12": ("texture", 256, 8, 1, 8, 12),   # the shipped width, 32-channel grid
    "h96-nogrid-b1-8x8x6": ("baseline", 96, 0, 1, 8, 6),     # a width without grid
}


def T(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float32), device=DEV)


@functools.lru_cache(maxsize=None)
def _state(kind, H, grid):
    spec = proc.model_spec(kind, hidden_dim=H, grid_size=grid, z_dim=8)
    return spec, proc.make_state_dict(spec, seed=6, sigma_gain=60.0, with_mapping=False)


@functools.lru_cache(maxsize=None)
def _model(kind, H, grid, balanced=False):
    """balanced: the sigma bias moved by the median sigma of the seed-0 samples of the 8 x 8 x 6 shape, so that about half of the samples
    are kept (the models as they come keep nearly every sample: lists at full length, but next to nothing skipped)"""
    spec, sd = _state(kind, H, grid)
    if balanced:
        sd = dict(sd)
        sd["final_layer.bias"] = sd["final_layer.bias"] - np.float32(_sigma_shift(kind, H, grid))
    return native.NativeModel(sd, spec, DEV, "f16x3")


def _sigma_shift(kind, H, grid):
    """the bias shift of the balanced model (the same measurement: deterministic)"""
    spec, sd = _state(kind, H, grid)
    a = _inputs(spec, 1, 8, 6, 0)
    return _model(kind, H, grid).siren_forward_rays(a["o"], a["d"], a["z"], *_tf(a))[..., -1].median().item()


def _inputs(spec, B, S, N, seed):
    film = proc.film_params(spec, B, seed=seed)
    torch.manual_seed(12 + seed)
    o, d, z, _, _ = VR.sample_rays(B, N, DEV, 12, (S, S), 0.88, 1.12, 0.3, 0.155, np.pi / 2, np.pi / 2, "gaussian")
    u = torch.rand((B * S * S, N), device=DEV)
    return dict(o=o, d=d, z=z, u=u, film={k: T(film[k]) for k in ("freq_geo", "phase_geo", "freq_app", "phase_app")})


def _tf(a):
    return tuple(a["film"][k] for k in ("freq_geo", "phase_geo", "freq_app", "phase_app"))


def _render(nat, a, mode, opts=None, nc=None, nf=None, timing=None):
    opts = opts or _lib.composite_opts("relu", 0.0, fill_mode="seg_padding_background", fill_color="black")
    with native.render_split(mode), native.render_fusion("off"), native.phase_timing() as t:
        out = nat.render(a["o"], a["d"], a["z"], a["u"], nc, nf, *_tf(a), opts, hierarchical=True, want_weights=True, want_wsum=True)
        torch.cuda.synchronize()
    if timing is not None:
        timing.update(t.calls)
    return out


def _kept(nat, a):
    """kept samples per image, from the dense kernel's sigma rows"""
    B = a["z"].shape[0]
    sig = nat.siren_forward_rays(a["o"], a["d"], a["z"], *_tf(a))[..., -1]
    return [int(v) for v in (~(sig <= 0)).reshape(B, -1).sum(1)]


def _assert_same(dense, split, what):
    for name, x, y in zip(NAMES, dense, split):
        assert torch.equal(torch.isnan(x), torch.isnan(y)), (what, name, "NaNs sit in the same places")
        assert torch.equal(torch.nan_to_num(x, nan=-7.0), torch.nan_to_num(y, nan=-7.0)), (what, name, float((x - y).abs().nan_to_num().max()))


def _seeded_inputs(nat, spec, B, S, N):
    """the first input seed whose kept counts make the case meaningful: a count that is no multiple of 16, a count of at least 17"""
    for seed in range(8):
        a = _inputs(spec, B, S, N, seed)
        k = _kept(nat, a)
        if any(c % 16 for c in k) and any(c >= 17 for c in k):
            return a, k
    raise AssertionError("no seed in 0..7 gives a partial tile and a list of at least 17 samples")


@pytest.mark.parametrize("balanced", [False, True], ids=["sigma-as-is", "sigma-balanced"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_split_route_equals_the_dense_route(shape, balanced):
    kind, H, grid, B, S, N = SHAPES[shape]
    spec, _ = _state(kind, H, grid)
    nat = _model(kind, H, grid, balanced)
    a, k = _seeded_inputs(nat, spec, B, S, N)
    print(f"[split] {shape}: kept per image {k} of {S * S * N}")
    assert any(c % 16 for c in k) and any(c >= 17 for c in k), k
    if balanced:        # a case that really skips: between a quarter and three quarters of the samples kept
        assert S * S * N * B // 4 <= sum(k) <= 3 * S * S * N * B // 4, k
    calls = {}
    dense = _render(nat, a, "off")
    split = _render(nat, a, "force", timing=calls)
    assert calls.get("siren_density") == 1 and calls.get("siren_colour") == 1, calls
    _assert_same(dense, split, shape)
    auto_calls = {}
    _assert_same(dense, _render(nat, a, "auto", timing=auto_calls), shape + "-auto")


@pytest.mark.parametrize("extreme", ["every-sample-kept", "no-sample-kept"])
def test_capacity_edge_and_empty_lists(extreme):
    kind, H, grid, B, S, N = SHAPES["h32-grid8-b2-8x8x6"]
    spec, sd = _state(kind, H, grid)
    sd2 = dict(sd)
    sd2["final_layer.bias"] = np.full_like(sd["final_layer.bias"], 1e6 if extreme == "every-sample-kept" else -1e6)
    nat = native.NativeModel(sd2, spec, DEV, "f16x3")
    a = _inputs(spec, B, S, N, 0)
    k = _kept(nat, a)
    assert k == [S * S * N if extreme == "every-sample-kept" else 0] * B, k      # count = R N (the capacity edge) / 0 (no colour work at all)
    _assert_same(_render(nat, a, "off"), _render(nat, a, "force"), extreme)


CONDITIONS = {
    "softplus": dict(opts=("softplus", 0.0, False)),
    "last_back": dict(opts=("relu", 0.0, True)),
    "final-noise": dict(opts=("relu", 0.3, False), noise=True),
}


@pytest.mark.parametrize("cond", list(CONDITIONS))
def test_route_is_refused_where_its_conditions_do_not_hold(cond):
    kind, H, grid, B, S, N = SHAPES["h32-grid8-b2-8x8x6"]
    spec, _ = _state(kind, H, grid)
    nat = _model(kind, H, grid)
    a = _inputs(spec, B, S, N, 0)
    clamp, noise_std, last_back = CONDITIONS[cond]["opts"]
    opts = _lib.composite_opts(clamp, noise_std, last_back=last_back)
    nc = nf = None
    if CONDITIONS[cond].get("noise"):
        torch.manual_seed(3)
        nc, nf = torch.randn((B * S * S, N), device=DEV), torch.randn((B * S * S, 2 * N), device=DEV)
    with pytest.raises(_lib.FenerfError) as e:
        _render(nat, a, "force", opts, nc, nf)
    assert e.value.code == _lib.E_UNSUPPORTED
    calls = {}
    auto = _render(nat, a, "auto", opts, nc, nf, timing=calls)
    assert "siren_density" not in calls and "siren_colour" not in calls, calls
    _assert_same(_render(nat, a, "off", opts, nc, nf), auto, cond)


def test_coarse_noise_alone_keeps_the_route():
    """noise on the coarse composite only moves the resampled depths: noise_final == NULL leaves alpha = 0 for sigma <= 0 in the pixels"""
    kind, H, grid, B, S, N = SHAPES["h32-grid8-b2-8x8x6"]
    spec, _ = _state(kind, H, grid)
    nat = _model(kind, H, grid, True)
    a = _inputs(spec, B, S, N, 0)
    torch.manual_seed(3)
    nc = torch.randn((B * S * S, N), device=DEV)
    opts = _lib.composite_opts("relu", 0.3)
    _assert_same(_render(nat, a, "off", opts, nc, None), _render(nat, a, "force", opts, nc, None), "coarse-noise")


@pytest.mark.parametrize("what", ["ray-direction", "freq_app-of-one-image", "grid-voxel", "colour-layer-weight"])
def test_nonfinite_colour_inputs_reach_the_same_pixels(what):
    kind, H, grid, B, S, N = SHAPES["h32-grid8-b2-8x8x6"]
    spec, sd = _state(kind, H, grid)
    nat = _model(kind, H, grid, True)
    sd = dict(sd)
    sd["final_layer.bias"] = sd["final_layer.bias"] - np.float32(_sigma_shift(kind, H, grid))
    a = _inputs(spec, B, S, N, 0)
    img, ray = 1, 21
    if what == "ray-direction":
        a["d"] = a["d"].clone()
        a["d"][img, ray, 1] = float("nan")
    elif what == "freq_app-of-one-image":
        a["film"]["freq_app"] = a["film"]["freq_app"].clone()
        a["film"]["freq_app"][img, 5] = float("nan")
    else:
        sd2 = dict(sd)
        if what == "grid-voxel":
            g = sd["spatial_embeddings"].copy()
            g[0, 3, grid // 2, grid // 2, grid // 2] = np.nan
            sd2["spatial_embeddings"] = g
        else:
            w = sd["color_layer_sine.1.layer.weight"].copy()
            w[4, 9] = np.nan
            sd2["color_layer_sine.1.layer.weight"] = w
        nat = native.NativeModel(sd2, spec, DEV, "f16x3")
    dense = _render(nat, a, "off")
    nan_pixels = torch.isnan(dense[0]).any(-1)
    assert bool(nan_pixels.any()), (what, "the dense route has NaN pixels to lose")
    if what == "ray-direction":
        assert bool(nan_pixels[img, ray])
    if what == "freq_app-of-one-image":
        assert bool(nan_pixels[img].any()) and not bool(nan_pixels[1 - img].any())
    if what == "colour-layer-weight":
        assert bool(nan_pixels[0].any()) and bool(nan_pixels[1].any())
    _assert_same(dense, _render(nat, a, "force"), what)


def test_second_render_on_the_same_workspace_is_its_own():
    """stale counts / lists / parked trunk outputs of an earlier render on the same workspace must not reach the next one"""
    kind, H, grid, B, S, N = SHAPES["h32-grid8-b2-8x8x6"]
    spec, _ = _state(kind, H, grid)
    nat = _model(kind, H, grid, True)
    a1, a2 = _inputs(spec, B, S, N, 1), _inputs(spec, B, S, N, 2)
    assert _kept(nat, a1) != _kept(nat, a2)
    dense2 = [t.clone() for t in _render(nat, a2, "off")]
    _render(nat, a1, "force")
    _assert_same(dense2, _render(nat, a2, "force"), "second render")
