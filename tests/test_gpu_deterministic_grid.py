"""The deterministic feature-grid gradient (include/fenerf.h FENERF_GRID_GRAD_DETERMINISTIC, fenerf_grid_backward_det): bit for bit against
its numpy restatement (fenerf_amd/grid_det_emulation.py), and the generator step under torch.use_deterministic_algorithms(True) on the
H = 256 + 96^3 model -- the same bits run to run, for any chunking, through the render ABI and the Python orchestration, one- and two-node,
dense and sparse -- within the fp64 bounds the atomics route meets."""
import contextlib
import functools
import warnings

import numpy as np
import pytest
import torch

from conftest import kwargs_from_golden, load_golden, spec_from_golden, state_from_golden, film_from_golden
from fenerf_amd import _lib, native, procedural as proc
from fenerf_amd import grid_det_emulation as E
from fenerf_amd.generators import autograd as GA
from fenerf_amd.generators import generators as G
from fenerf_amd.generators import volumetric_rendering as VR
from fenerf_amd.siren import autograd as SA
from fenerf_amd.siren import siren as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


def N_(t):
    return t.detach().cpu().numpy()


def _rel_err(got, ref):
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-12))


@contextlib.contextmanager
def deterministic(on=True, warn_only=False):
    old = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled())
    torch.use_deterministic_algorithms(on, warn_only=warn_only)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(old[0], warn_only=old[1])


# ---------------------------------------------------------------------------------------------------------------------------------------
# fenerf_grid_backward_det == its numpy restatement, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------------------
def _rows(case, n=16000, grid=8, seed=0):
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-0.14, 0.14, (n, 3)).astype(np.float32)            # the box is +-0.12: points and corners outside it
    nodes = rng.integers(0, grid, (n // 8, 3))
    pts[:n // 8] = ((2.0 * nodes / (grid - 1) - 1.0) / float(E.BOX_SCALE)).astype(np.float32)     # on (or next to) grid nodes
    d_e = rng.normal(size=(n, 32)).astype(np.float32)
    d_e[rng.random(n) < 0.4] = 0                                           # all-zero rows
    if case == "hot":                                                     # one voxel hit by 12,000 rows
        pts[2000:14000] = np.float32([0.013, -0.021, 0.034])
    elif case == "tiny":
        d_e *= np.float32(1e-30)
    elif case == "huge":
        d_e *= np.float32(1e30)
    elif case == "nonfinite":
        r = rng.choice(n, 40, replace=False)
        d_e[r[:20], rng.integers(0, 32, 20)] = np.nan
        d_e[r[20:30]] = np.inf
        d_e[r[30:], 5] = -np.inf
    return pts, d_e


def _grid_model(grid=8):
    spec = proc.model_spec("texture", hidden_dim=32, grid_size=grid, z_dim=8)
    sd = proc.make_state_dict(spec, seed=1, sigma_gain=30.0, with_mapping=False)
    return native.NativeModel(sd, spec, DEV, "f32", differentiable=True)


@pytest.mark.parametrize("case", ["random", "hot", "tiny", "huge", "nonfinite"])
def test_grid_backward_det_equals_the_numpy_emulation(case):
    nat = _grid_model()
    pts, d_e = _rows(case)
    n = pts.shape[0]
    for dense_rows in (n, 3 * n + 5):
        got = N_(nat.grid_backward_det(T(pts), T(d_e), dense_rows))
        ref = E.grid_backward_det(pts, d_e, nat.grid_shape, dense_rows)
        assert np.array_equal(np.isnan(got), np.isnan(ref)), (case, int(np.isnan(got).sum()), int(np.isnan(ref).sum()))
        assert np.array_equal(got, ref, equal_nan=True), (case, dense_rows, float(np.nanmax(np.abs(got - ref))))
        perm = np.random.default_rng(7).permutation(n)
        again = N_(nat.grid_backward_det(T(pts[perm]), T(d_e[perm]), dense_rows))
        assert np.array_equal(got.view(np.uint32), again.view(np.uint32)), "order of the rows"
    assert np.abs(np.nan_to_num(got)).max() > 0
    if case == "nonfinite":          # NaN at exactly the voxel-channels the non-finite values touch
        bad = np.zeros(got.shape, dtype=bool).reshape(-1, 32)
        for ok, vox, _ in E.corners(pts, nat.grid_shape):
            r, c = np.nonzero(~np.isfinite(d_e) & ok[:, None])
            bad[vox[r], c] = True
        assert np.array_equal(np.isnan(got).reshape(-1, 32), bad) and bad.any()
    else:
        assert np.isfinite(got).all()
    print(f"[det-grid] fenerf_grid_backward_det [{case}]: {n} rows == numpy emulation bit for bit, any row order")


def test_grid_backward_det_without_rows_is_zero_and_refusals():
    nat = _grid_model()
    empty = torch.empty((0, 32), dtype=torch.float32, device=DEV)
    g = nat.grid_backward_det(empty[:, :3], empty, 1)
    assert g.shape == nat.grid_shape + (32,) and not g.any()
    l = _lib.lib()
    try:
        assert nat.set_grid_grad_mode(True) == _lib.GRID_GRAD_ATOMIC and nat.grid_grad_mode == _lib.GRID_GRAD_DETERMINISTIC
        assert l.fenerf_siren_backward_fuses_grid(nat._h) == 0
        pts, d_e = _rows("random", n=64)
        with pytest.raises(_lib.FenerfError, match="fenerf_grid_backward_det"):
            nat.grid_backward(T(pts), T(d_e), nat.grid_shape)          # accumulates per call: refused, never silently atomic
    finally:
        nat.set_grid_grad_mode(False)
    assert l.fenerf_model_set_grid_grad_mode(nat._h, 7) < 0 and nat.grid_grad_mode == _lib.GRID_GRAD_ATOMIC


# ---------------------------------------------------------------------------------------------------------------------------------------
# generator steps on the H = 256 + 96^3 model
# ---------------------------------------------------------------------------------------------------------------------------------------
KW = dict(img_size=32, fov=12, ray_start=0.88, ray_end=1.12, num_steps=12, h_stddev=0.3, v_stddev=0.155, h_mean=np.pi / 2, v_mean=np.pi / 2,
          hierarchical_sample=True, sample_dist="gaussian", clamp_mode="relu", nerf_noise=0.2, last_back=False)
B = 2
RN = KW["img_size"] ** 2 * KW["num_steps"]


def _generator(precision):
    torch.manual_seed(0)                  # the mapping networks the procedural state does not set
    spec = proc.model_spec("texture", hidden_dim=256, grid_size=96, z_dim=8)
    sd = proc.make_state_dict(spec, seed=0, sigma_gain=2000.0, with_mapping=False)
    mod = S.TextureEmbeddingPiGAN128SEMANTICDISENTANGLE(hidden_dim=256, z_geo_dim=8, z_app_dim=8, output_dim=22)
    tsd = {k: torch.from_numpy(v) for k, v in sd.items()}
    mod.spatial_embeddings = torch.nn.Parameter(tsd["spatial_embeddings"].clone())
    mod.load_state_dict(tsd, strict=False)
    mod.precision = precision
    gen = G.DoubleImplicitGenerator3d(functools.partial(S.TextureEmbeddingPiGAN128SEMANTICDISENTANGLE, hidden_dim=256), 8, 8, 22)
    gen.siren = mod
    gen = gen.to(DEV)
    gen.device = torch.device(DEV); gen.siren.device = gen.device
    return gen, proc.film_params(spec, B, seed=4)


def _step(gen, film, seed=11, w_nan=False):
    film_t = {k: T(v).requires_grad_(True) for k, v in film.items()}
    for p_ in gen.siren.parameters():
        p_.grad = None
    torch.manual_seed(seed)
    px, _ = gen.forward_with_frequencies(film_t["freq_geo"], film_t["freq_app"], film_t["phase_geo"], film_t["phase_app"], **KW)
    w = torch.randn(px.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    if w_nan:
        w[0, :, 13, 17] = float("nan")
    (px * w).sum().backward()
    g = {k: N_(v.grad) for k, v in film_t.items()}
    g.update({k: N_(p_.grad) for k, p_ in gen.siren.named_parameters() if p_.grad is not None})
    return g


def _same(a, b, keys=None):
    keys = sorted(a) if keys is None else keys
    assert a.keys() == b.keys()
    return [k for k in keys if not np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32))]


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_generator_step_is_bit_reproducible_under_torch_deterministic(precision):
    gen, film = _generator(precision)
    mod = gen.siren
    old = (SA.BACKWARD_CHUNK_POINTS, GA.USE_RENDER_ABI)
    try:
        with deterministic():
            g0 = _step(gen, film)
            assert len(g0) == 37 and "spatial_embeddings" in g0
            assert mod.native_differentiable(DEV).grid_grad_mode == _lib.GRID_GRAD_DETERMINISTIC
            assert not _same(g0, _step(gen, film)), "run to run"
            for chunk in (2 * RN, 196608, 2048):
                SA.BACKWARD_CHUNK_POINTS = chunk
                assert not _same(g0, _step(gen, film), ["spatial_embeddings"]), f"chunk {chunk}"
            SA.BACKWARD_CHUNK_POINTS = old[0]
            GA.USE_RENDER_ABI = False
            assert not _same(g0, _step(gen, film)), "render ABI vs the Python orchestration"
            for abi in (False, True):
                GA.USE_RENDER_ABI = abi
                mod.split_backward = True
                for keep in (1, 3):
                    mod.split_keep_chunks = keep
                    SA.BACKWARD_CHUNK_POINTS = 2048 if keep == 3 else old[0]
                    g1 = _step(gen, film)
                    SA.BACKWARD_CHUNK_POINTS = old[0]
                    diff = _same(g0, g1) if keep == 1 else _same(g0, g1, ["spatial_embeddings"])
                    assert not diff, (f"split backward, abi {abi}, keep {keep}", diff)
                mod.split_backward = False
            GA.USE_RENDER_ABI = old[1]
            mod.sparse_backward = True
            gs = _step(gen, film)
            kept = GA.SparseHierarchicalRenderFunction.last_kept
            GA.SparseHierarchicalRenderFunction.verify()
            assert int(kept[0]) < kept[1]
            assert not _same(g0, gs, ["spatial_embeddings"]), ("dense vs sparse", _rel_err(gs["spatial_embeddings"], g0["spatial_embeddings"]))
            mod.sparse_backward = False
        # both switches off: the atomics route, reported by the model, within the usual distance of the deterministic gradient
        ga = _step(gen, film)
        assert mod.native_differentiable(DEV).grid_grad_mode == _lib.GRID_GRAD_ATOMIC
        assert _rel_err(ga["spatial_embeddings"], g0["spatial_embeddings"]) <= 1e-6
        assert not _same(g0, ga, [k for k in g0 if k != "spatial_embeddings"])
    finally:
        SA.BACKWARD_CHUNK_POINTS, GA.USE_RENDER_ABI = old
        mod.split_backward = mod.sparse_backward = False
    print(f"[det-grid] generator step [{precision}] under torch.use_deterministic_algorithms(True): 37 gradient tensors bit-identical run to run, "
          f"render ABI vs Python, one- vs two-node; grid gradient bit-identical over chunkings and dense vs sparse ({int(kept[0])} of {kept[1]} samples "
          f"kept); atomics route {_rel_err(ga['spatial_embeddings'], g0['spatial_embeddings']):.1e} away")


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_two_training_steps_reproduce_every_parameter(precision):
    def run():
        gen, film = _generator(precision)
        grid0 = N_(gen.siren.spatial_embeddings)
        params = [p_ for p_ in gen.siren.parameters() if p_.requires_grad]
        opt = torch.optim.Adam(params, lr=1e-3)
        with deterministic():
            for step in range(2):
                _step(gen, film, seed=11 + step)
                opt.step()
        res = {k: N_(p_) for k, p_ in gen.siren.named_parameters()}
        assert np.abs(res["spatial_embeddings"] - grid0).max() > 0
        return res
    a = run()
    b = run()
    assert not _same(a, b), "parameters after two G-steps + Adam"
    print(f"[det-grid] two G-steps + Adam + re-pack [{precision}] under torch.use_deterministic_algorithms(True): {len(a)} parameters bit-identical")


def test_deterministic_backward_attribute_and_alerts():
    gen, film = _generator("f16x3")
    mod = gen.siren
    try:
        mod.deterministic_backward = True                 # without torch's switch
        g_det = _step(gen, film)
        assert mod.native_differentiable(DEV).grid_grad_mode == _lib.GRID_GRAD_DETERMINISTIC
        mod.deterministic_backward = None
        _step(gen, film)
        assert mod.native_differentiable(DEV).grid_grad_mode == _lib.GRID_GRAD_ATOMIC
        mod.deterministic_backward = False                # the atomics route asked for under torch's switch: raise / warn, as torch does
        with deterministic(), pytest.raises(RuntimeError, match="not deterministic"):
            _step(gen, film)
        with deterministic(warn_only=True), warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            _step(gen, film)
        assert any("not deterministic" in str(w_.message) for w_ in caught)
        mod.deterministic_backward = None
        # a non-finite upstream gradient: the same non-finite voxel-channels as the atomics route
        g_nan_a = _step(gen, film, w_nan=True)["spatial_embeddings"]
        with deterministic():
            g_nan_d = _step(gen, film, w_nan=True)["spatial_embeddings"]
        assert not np.isfinite(g_nan_d).all()
        assert np.array_equal(~np.isfinite(g_nan_d), ~np.isfinite(g_nan_a))
        assert np.isfinite(g_det["spatial_embeddings"]).all()
    finally:
        mod.deterministic_backward = None


# ---------------------------------------------------------------------------------------------------------------------------------------
# the bounds the atomics route meets: reference autograd fixtures with a grid, and the 96^3 grid at full size against fp64
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "f16x3"])
@pytest.mark.parametrize("name,bound", [("tiny_texture_grad", 1.0e-4), ("tiny_texture_grad_trained", 8e-5), ("h96_texture_grad", 2.2e-3)])
def test_deterministic_grid_gradient_vs_reference_autograd(name, bound, precision):
    g = load_golden(name)
    spec = spec_from_golden(g)
    spec = dict(spec, z_dim=spec.get("z_dim", 16))
    H = spec["hidden_dim"]
    gen = G.DoubleImplicitGenerator3d(functools.partial(S.TextureEmbeddingPiGAN128SEMANTICDISENTANGLE, hidden_dim=H), spec["z_dim"], spec["z_dim"], 22)
    sd = proc.make_state_dict(dict(spec, map_hidden=256), seed=int(g["meta_seed"]) if "meta_seed" in g else 3,
                              sigma_gain=float(g["meta_sigma_gain"]) if "meta_sigma_gain" in g else 300.0)
    st = state_from_golden(g)
    if st is not None:
        sd.update(st[0])
    tsd = {k: torch.from_numpy(v) for k, v in sd.items()}
    gen.siren.spatial_embeddings = torch.nn.Parameter(tsd["spatial_embeddings"].clone())
    gen.siren.load_state_dict(tsd, strict=True)
    gen = gen.to(DEV).train()
    gen.siren.precision = precision
    gen.device = torch.device(DEV); gen.siren.device = gen.device
    f = film_from_golden(g, spec)
    tf = [T(f[k]).requires_grad_(True) for k in ("freq_geo", "phase_geo", "freq_app", "phase_app")]
    gen.draws = VR.RecordedDraws([g["rand_u_jitter"], g["rand_r_theta"], g["rand_r_phi"], g["rand_noise_coarse"], g["rand_u_fine"], g["rand_noise_fine"]])
    common = dict(img_size=int(g["meta_S"]), fov=12, ray_start=0.88, ray_end=1.12, num_steps=int(g["meta_N"]), h_stddev=0.3, v_stddev=0.155,
                  h_mean=np.pi * 0.5, v_mean=np.pi * 0.5, hierarchical_sample=True, sample_dist="gaussian", **kwargs_from_golden(g))
    with deterministic():
        px, _ = gen.forward_with_frequencies(tf[0], tf[2], tf[1], tf[3], **common)
        (px * T(g["loss_w"])).sum().backward()
    assert gen.siren.native_differentiable(DEV).grid_grad_mode == _lib.GRID_GRAD_DETERMINISTIC
    named = dict(gen.siren.named_parameters())
    e_grid = _rel_err(N_(named["spatial_embeddings"].grad), g["gparam_spatial_embeddings"])
    worst = max(_rel_err(N_(named[k[7:]].grad), g[k]) for k in g if k.startswith("gparam_"))
    print(f"[det-grid] {name}[{precision}] deterministic grid gradient vs the reference's autograd {e_grid:.2e} (worst of all tensors {worst:.2e})")
    assert e_grid <= bound and worst <= bound


def test_deterministic_grid_gradient_at_full_size_96cubed_grid():
    """test_gpu_parity.py's full-size check of the 96^3 grid gradient (786,432 points, the upstream gradient on a 2,048-ray slab) with the
    deterministic route: fp64 autograd of the slab alone within the same 6e-5, no stray voxel."""
    from oracle import fenerf_oracle_grad as OG
    spec = proc.model_spec("texture", hidden_dim=256, grid_size=96)
    sd = proc.make_state_dict(spec, seed=0, sigma_gain=2000.0, with_mapping=False)
    mod = S.TextureEmbeddingPiGAN128SEMANTICDISENTANGLE(hidden_dim=256, z_geo_dim=8, z_app_dim=8, output_dim=22)
    tsd = {k: torch.from_numpy(v) for k, v in sd.items()}
    mod.spatial_embeddings = torch.nn.Parameter(tsd["spatial_embeddings"].clone())
    mod.load_state_dict(tsd, strict=False)
    mod.precision = "f16x3"
    mod = mod.to(DEV)
    S_, N = 128, 24
    R = S_ * S_
    torch.manual_seed(0)
    o, d, z, _, _ = VR.sample_rays(1, N, DEV, 12, (S_, S_), 0.88, 1.12, 0.3, 0.155, np.pi / 2, np.pi / 2, "gaussian")
    zf = torch.sort(0.88 + 0.24 * torch.rand((1, R, N), device=DEV), -1)[0]
    pts = torch.cat([(o[:, :, None, :] + d[:, :, None, :] * zz[..., None]).reshape(1, R * N, 3) for zz in (z, zf)], 0)
    dirs = d[:, :, None, :].expand(1, R, N, 3).reshape(1, R * N, 3).expand(2, -1, -1).contiguous()
    film2 = {k: np.repeat(v, 2, 0) for k, v in proc.film_params(spec, 1, seed=0).items()}
    r0, r1 = 7168, 9216
    rng = np.random.default_rng(5)
    g_slab = rng.normal(size=(2, (r1 - r0) * N, 22)).astype(np.float32)
    g_slab[..., -1] *= 1e-3
    g_out = torch.zeros((2, R * N, 22), device=DEV)
    g_out[:, r0 * N:r1 * N] = T(g_slab)
    t64 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    sd64 = {"spatial_embeddings": t64(sd["spatial_embeddings"]).requires_grad_(True)}
    sd64.update({k: t64(v) for k, v in sd.items() if k != "spatial_embeddings"})
    film64 = {k: t64(v) for k, v in film2.items()}
    p_slab, d_slab = N_(pts[:, r0 * N:r1 * N]), N_(dirs[:, r0 * N:r1 * N])
    for s0 in range(0, p_slab.shape[1], 8192):
        sl = slice(s0, s0 + 8192)
        ref = OG.siren_forward(sd64, spec, t64(p_slab[:, sl]), t64(d_slab[:, sl]), film64["freq_geo"], film64["phase_geo"], film64["freq_app"], film64["phase_app"])
        (ref * t64(g_slab[:, sl])).sum().backward()
    g_ref = sd64["spatial_embeddings"].grad.numpy()
    touched_ref = np.abs(g_ref).max(1) > 0
    film_t = {k: T(v).requires_grad_(True) for k, v in film2.items()}
    with deterministic():
        out = mod.forward_with_frequencies_phase_shifts(pts, film_t["freq_geo"], film_t["freq_app"], film_t["phase_geo"], film_t["phase_app"], dirs)
        (out * g_out).sum().backward()
    assert mod.native_differentiable(DEV).grid_grad_mode == _lib.GRID_GRAD_DETERMINISTIC
    g_nat = N_(mod.spatial_embeddings.grad)
    touched = np.abs(g_nat).max(1) > 0
    e_grid = _rel_err(g_nat, g_ref)
    print(f"[det-grid] 96^3 grid gradient at full size, deterministic route: relative error vs fp64 {e_grid:.2e}, {int(touched.sum())} voxels touched "
          f"(fp64: {int(touched_ref.sum())})")
    assert not (touched & ~touched_ref).any() and e_grid <= 6e-5
