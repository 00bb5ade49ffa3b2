"""The forward ray tail on the GPU (-m gpu): alpha compositing, the fine / coarse merge, inverse-CDF resampling and ray setup
(fenerf_amd/csrc/fenerf_composite.hip, fenerf_composite_ray.h) at every slot edge, channel pass and flag.

  resample / sample_pdf    bit for bit against the numpy emulation (fenerf_amd/resample_emulation.py), which tests/test_ray_tail_cpu.py holds
                           to the fp64 oracle on the same arrays
  composite / merge        against O.fancy_integration in fp64 on the fp32 inputs: err <= 4 e32 + 8 * 2^-24 * max(1, max|ref|), e32 the fp32
                           numpy oracle's own error on the same inputs (the factor 4: scan-tree product order, device expf / log1pf, the
                           two-lane channel sum), never above the ceilings the suite already uses; fill decisions on ALL rays; sort exact
  ray setup                the same bound against the fp64 oracle fed the float32-clamped pitch; z bit for bit against the CPU statement

The inputs come from tests/ray_tail_cases.py, where the CPU tests establish what they must hold (margins to the fill threshold and to the
resampling clamp, no overflow) on the reference alone."""
import math

import numpy as np
import pytest
import torch

import ray_tail_cases as RC
from conftest import load_golden
from fenerf_amd import _lib, native, procedural as proc, resample_emulation as RE
from fenerf_amd.generators import volumetric_rendering as VR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32


def T(a):
    return torch.as_tensor(np.array(a, dtype=np.float32), device=DEV)      # a copy: the cases are read-only and shared


def N_(t):
    return t.detach().cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return a.view(np.uint32)


def _assert_same_bits(tag, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    same = _bits(got) == _bits(want)
    if not same.all():
        idx = np.argwhere(~same)
        first = tuple(idx[0])
        raise AssertionError(f"{tag}: {len(idx)} of {same.size} values differ in bits; first at {first}: got {got[first]!r} ({_bits(got)[first]:#010x}), "
                             f"want {want[first]!r} ({_bits(want)[first]:#010x}); rays {sorted(set(idx[:, 0].tolist()))}")


# ---------------------------------------------------------------------------------------------------
# a. resample and sample_pdf equal the emulation bit for bit
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", RC.RESAMPLE_N)
def test_resample_equals_emulation_bit_for_bit(N):
    z, w, u = RC.resample_case(N)
    want, _ = RE.resample(z, w, u)
    got = N_(native.resample(T(z), T(w), T(u)))
    _assert_same_bits(f"resample N={N}", got, want)


@pytest.mark.parametrize("K,NS", RC.SAMPLE_PDF_SHAPES)
def test_sample_pdf_equals_emulation_bit_for_bit(K, NS):
    bins, w, u = RC.sample_pdf_case(K, NS)
    want, _ = RE.sample_pdf(bins, w, u)
    got = N_(native.sample_pdf(T(bins), T(w), T(u)))
    _assert_same_bits(f"sample_pdf K={K} NS={NS}", got, want)


# ---------------------------------------------------------------------------------------------------
# b. the resample fused into the coarse composite of fenerf_render_forward equals the stand-alone kernel
# ---------------------------------------------------------------------------------------------------
_tiny = {}


def _tiny_model():
    if not _tiny:
        spec = proc.model_spec("texture", hidden_dim=32, grid_size=5, z_dim=8)
        sd = proc.make_state_dict(spec, seed=2, sigma_gain=40.0, with_mapping=False)
        film = proc.film_params(spec, 1, seed=2)
        _tiny["nat"] = native.NativeModel(sd, spec, DEV, "f32")
        _tiny["film"] = tuple(T(film[k]) for k in ("freq_geo", "phase_geo", "freq_app", "phase_app"))
    return _tiny["nat"], _tiny["film"]


@pytest.mark.parametrize("N", [65, 67, 130, 258])
def test_fused_resample_equals_the_separate_entry_points(N):
    """fenerf_render_forward in four launches (render_fusion "off") resamples inside the coarse composite's wave (composite_ray with z_fine);
    the same pipeline through siren_forward_rays, composite, resample, siren_forward_rays, merge_composite uses resample_kernel.  Same
    arithmetic, so pixels, depth, weights and weights_sum are the same bits."""
    nat, tf = _tiny_model()
    B, S = 1, 3
    R = S * S
    rng = np.random.default_rng(7000 + N)
    z_cam = (-torch.ones(1) / np.tan((2 * math.pi * 12 / 360) / 2)).item()
    o, d, z, _, _ = native.ray_setup(B, S, N, z_cam, 0.88, 1.12, T(rng.random((B, R, N, 1))), T(np.array([math.pi / 2 + 0.2])), T(np.array([math.pi / 2 - 0.1])))
    u = T(rng.random((B * R, N)))
    opts = _lib.composite_opts("relu")
    with native.render_fusion("off"):
        rgb, depth, w, ws = nat.render(o, d, z, u, None, None, *tf, opts, hierarchical=True, want_weights=True, want_wsum=True)
    coarse = nat.siren_forward_rays(o, d, z, *tf)
    _, _, cw, _ = native.composite(coarse, z, None, opts)
    zf = native.resample(z.reshape(B * R, N), cw.reshape(B * R, N), u)
    fine = nat.siren_forward_rays(o, d, zf.reshape(B, R, N), *tf)
    rgb2, depth2, w2, ws2, _ = native.merge_composite(fine.reshape(B * R, N, -1), coarse.reshape(B * R, N, -1), zf, z.reshape(B * R, N), None, opts)
    torch.cuda.synchronize()
    assert np.isfinite(N_(rgb)).all() and (N_(ws) > 0).any()
    _assert_same_bits(f"fused N={N} weights", N_(w).reshape(B * R, 2 * N), N_(w2))
    _assert_same_bits(f"fused N={N} wsum", N_(ws).reshape(B * R), N_(ws2))
    _assert_same_bits(f"fused N={N} depth", N_(depth).reshape(B * R), N_(depth2))
    _assert_same_bits(f"fused N={N} pixels", N_(rgb).reshape(B * R, -1), N_(rgb2))


# ---------------------------------------------------------------------------------------------------
# c. composite forward against fp64
# ---------------------------------------------------------------------------------------------------
def _opts(flags, fill_mode=None, fill_color="black"):
    clamp, ns, lb, wb, bb = flags
    return _lib.composite_opts(clamp, ns, lb, wb, bb, fill_mode, fill_color)


def _noise(noise, flags):
    return T(noise) if flags[1] != 0 else None


def _check_values(tag, got, r64, r32, rows=None, names=("rgb", "depth", "weights", "wsum")):
    """every output within 4 e32 + 8 * 2^-24 * max(1, max|ref|) of fp64 (and the suite's ceiling) -> list of failures"""
    bad = []
    for name in names:
        g, a, b = (np.asarray(x[name]) for x in (got, r64, r32))
        assert g.shape == a.shape == b.shape, (tag, name, g.shape, a.shape, b.shape)
        assert g.dtype == np.float32 and a.dtype == np.float64 and b.dtype == np.float32
        if rows is not None:
            g, a, b = g[rows], a[rows], b[rows]
        err, e32 = RC.max_err(g, a), RC.max_err(b, a)
        bound = RC.value_bound(name, e32, a)
        print(f"[parity] {tag} {name}: err {err:.3e}  e32 {e32:.3e}  err/e32 {err / e32 if e32 else float('nan'):.2f}  bound {bound:.3e}")
        if not (np.isfinite(g).all() and err <= bound):
            bad.append(f"{tag} {name}: err {err:.3e} > bound {bound:.3e} (e32 {e32:.3e})")
    return bad


def _composite(rs, z, noise, flags, fill_mode=None, fill_color="black", **kw):
    rgb, depth, w, ws = native.composite(T(rs), T(z), _noise(noise, flags), _opts(flags, fill_mode, fill_color), **kw)
    return dict(rgb=N_(rgb), depth=N_(depth), weights=N_(w) if w is not None else None, wsum=N_(ws) if ws is not None else None)


def _composite_value_case(M, C, flags, BR=9):
    rs, z, noise = RC.composite_case(M, C, BR)
    got = _composite(rs, z, noise, flags)
    tag = f"composite M={M} C={C} {RC.flags_id(flags)}"
    bad = _check_values(tag, got, RC.oracle_composite(rs, z, noise, flags, np.float64), RC.oracle_composite(rs, z, noise, flags, np.float32))
    lean = _composite(rs, z, noise, flags, want_weights=False, want_wsum=False)      # the optional outputs do not change the others
    assert lean["weights"] is None and lean["wsum"] is None
    _assert_same_bits(tag + " rgb without weights / wsum", lean["rgb"], got["rgb"])
    _assert_same_bits(tag + " depth without weights / wsum", lean["depth"], got["depth"])
    return bad


@pytest.mark.parametrize("M,C,flags", RC.composite_rotation(), ids=lambda v: RC.flags_id(v) if isinstance(v, tuple) else str(v))
def test_composite_forward_vs_fp64(M, C, flags):
    bad = _composite_value_case(M, C, flags)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("M", RC.FULL_PRODUCT_M)
def test_composite_forward_every_flag_set_vs_fp64(M):
    """(relu | softplus) x noise_std x last_back x (none | white_back | black_back) on rays of two and three 64-sample slots, C = 36: the
    second channel pass, noise by sorted position, softplus across the slot carry, last_back in slot 1 / 2"""
    bad = []
    for flags in RC.FLAG_SETS:
        bad += _composite_value_case(M, 36, flags)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("M", RC.FILL_M)
def test_composite_fill_modes_vs_fp64(M):
    flags = ("relu", 0.0, False, False, False)
    bad = []
    for mode, color, c_forced in RC.FILL_MODES:
        C = c_forced or RC.fill_channels(M)
        rs, z = RC.graded_case(M, C)
        tag = f"fill M={M} C={C} {mode}/{color}"
        got = _composite(rs, z, None, flags, mode, color)
        r64 = RC.oracle_composite(rs, z, None, flags, np.float64, mode, color)
        r32 = RC.oracle_composite(rs, z, None, flags, np.float32, mode, color)
        low = r64["wsum"] < 0.9                                            # fp64's decision; every ray is > 1e-4 away from 0.9 (CPU test)
        assert 3 <= low.sum() <= len(low) - 3
        pad = mode in ("seg_padding_background", "eval_seg_padding_background")
        filled = low & (mode != "weight") & (not pad or color in _lib.FILL_COLORS)
        assert got["rgb"].shape == (len(low), C if pad else C - 1) == r64["rgb"].shape
        if pad:                                                            # the prepended background channel: 1 on filled rays, else 0
            assert np.array_equal(got["rgb"][:, 0], filled.astype(F)), (tag, got["rgb"][:, 0], filled)
            want = F(_lib.FILL_COLORS.get(color, 0.0))
            assert (got["rgb"][filled, 1:] == want).all(), tag            # exact
        elif mode == "eval_white_back":
            assert (got["rgb"][filled] == F(1)).all() and not (got["rgb"][~filled] == F(1)).all(axis=-1).any(), tag
        if filled.any():
            np.testing.assert_array_equal(got["rgb"][filled].astype(np.float64), r64["rgb"][filled].astype(F).astype(np.float64), err_msg=tag)
        bad += _check_values(tag + " unfilled rays", got, r64, r32, rows=~filled, names=("rgb",))
        bad += _check_values(tag, got, r64, r32, names=("depth", "weights", "wsum"))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("BR,M,flags", [(4 * 8192 + 5, 2, ("softplus", 0.5, True, True, False)), (2 * 8192 + 3, 513, ("relu", -0.3, True, False, True))],
                         ids=["4-waves-M2", "2-waves-M513"])
def test_composite_grid_stride_vs_fp64(BR, M, flags):
    """more rays than 8192 workgroups hold (four waves each, two for rays of more than 512 samples): the grid-stride ray loop; all rays"""
    bad = _composite_value_case(M, 2, flags, BR)
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------
# d. merge composite forward
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,C,flag_index", RC.merge_rotation())
def test_merge_composite_forward_vs_fp64(N, C, flag_index):
    fine, coarse, zf, zc, noise = RC.merge_case(N, C, flag_index)
    flags, fill_mode, fill_color = RC.merge_flags(flag_index)
    tag = f"merge N={N} C={C} {RC.flags_id(flags)}{' ' + fill_mode if fill_mode else ''}"
    rgb, depth, w, ws, zs = native.merge_composite(T(fine), T(coarse), T(zf), T(zc), _noise(noise, flags), _opts(flags, fill_mode, fill_color))
    got = dict(rgb=N_(rgb), depth=N_(depth), weights=N_(w), wsum=N_(ws))
    r64 = RC.oracle_merge(fine, coarse, zf, zc, noise, flags, np.float64, fill_mode, fill_color)
    r32 = RC.oracle_merge(fine, coarse, zf, zc, noise, flags, np.float32, fill_mode, fill_color)
    # the sort is exact and stable: cat([fine, coarse]) in argsort(kind="stable") order, ties by source index (fine first)
    assert np.array_equal(N_(zs), r32["z_sorted"]) and np.array_equal(r32["z_sorted"].astype(np.float64), r64["z_sorted"]), tag
    filled = np.zeros(len(zf), dtype=bool)
    if fill_mode:
        filled = r64["wsum"] < 0.9                                         # every ray > 1e-4 away from 0.9 (CPU test)
        assert filled.any() and not filled.all()
        assert np.array_equal(got["rgb"][:, 0], filled.astype(F)), (tag, got["rgb"][:, 0], filled)
        assert (got["rgb"][filled, 1:] == F(_lib.FILL_COLORS[fill_color])).all(), tag
    bad = _check_values(tag, got, r64, r32, rows=~filled, names=("rgb",)) + _check_values(tag, got, r64, r32, names=("depth", "weights", "wsum"))
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------
# e. ray setup against fp64
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,N,fov,ray_range", RC.RAY_SETUP_CASES)
def test_ray_setup_vs_fp64(S, N, fov, ray_range):
    """pitch and yaw bit for bit; origins, dirs and z within 4 e32 + 8 * 2^-24 * max(1, max|ref|) of the fp64 oracle; z bit for bit the
    CPU statement VR.sample_rays(..., "cpu").
    The last comparison depends on the host: the CPU statement's depths are torch.linspace's, which ATen's AVX2 and AVX-512 kernels round
    once per element (a fused multiply-add), as the kernel does.  Under ATEN_CPU_CAPABILITY=default (no FMA) torch.linspace(0.1, 5, 12)
    rounds the product on its own and the (3, 12, 12, (0.1, 5)) case differs by one ulp at sample 5.  The host-independent pin of the
    depths' rounding is test_ray_setup_depths_are_the_references_bits below."""
    B = 3
    u = RC.ray_setup_jitter(S, N)
    z_cam = (-torch.ones(1) / np.tan((2 * math.pi * fov / 360) / 2)).item()          # as sample_rays hands it over
    o, d, z, pitch, yaw = (N_(t) for t in native.ray_setup(B, S, N, z_cam, ray_range[0], ray_range[1], T(u), T(RC.RAY_THETA), T(RC.RAY_PHI)))
    want_pitch = RC.clamped_pitch(RC.RAY_PHI)
    _assert_same_bits("pitch", pitch.reshape(B), want_pitch)
    _assert_same_bits("yaw", yaw.reshape(B), RC.RAY_THETA)
    # the fp64 oracle on THAT float32 pitch
    r64 = RC.oracle_ray_setup(S, N, fov, ray_range, u, RC.RAY_THETA, want_pitch, np.float64)
    r32 = RC.oracle_ray_setup(S, N, fov, ray_range, u, RC.RAY_THETA, want_pitch, np.float32)
    bad = []
    for name, g, a, b in zip(("origins", "dirs", "z"), (o, d, z), r64, r32):
        assert g.shape == a.shape == b.shape and g.dtype == np.float32 and a.dtype == np.float64 and b.dtype == np.float32
        err, e32 = RC.max_err(g, a), RC.max_err(b, a)
        bound = 4 * e32 + 8 * RC.EPS24 * max(1.0, float(np.abs(a).max()))
        print(f"[parity] ray_setup S={S} N={N} fov={fov} {ray_range} {name}: err {err:.3e}  e32 {e32:.3e}  "
              f"err/e32 {err / e32 if e32 else float('nan'):.2f}  bound {bound:.3e}")
        if not (np.isfinite(g).all() and err <= bound):
            bad.append(f"{name}: err {err:.3e} > bound {bound:.3e} (e32 {e32:.3e})")
    assert not bad, "\n".join(bad)
    # z: bit for bit the project's CPU statement fed the same jitter
    z_cpu = VR.sample_rays(B, N, "cpu", fov, (S, S), ray_range[0], ray_range[1], 0.0, 0.0, 0.3, 1.0, "mean", draws=VR.RecordedDraws([u]))[2]
    _assert_same_bits("z against sample_rays on the CPU", z, N_(z_cpu))


@pytest.mark.parametrize("name", ["tiny_texture_fwd", "h256_texture_16x16_n24_trained"])
def test_ray_setup_depths_are_the_references_bits(name):
    """the jittered depths the reference recorded, bit for bit (with a separately rounded product, sample 9 of 24 is one ulp off)"""
    g = load_golden(name)
    B, R, N = g["st_z_coarse"].shape[:3]
    S = int(round(math.sqrt(R)))
    z = native.ray_setup(B, S, N, -9.5, 0.88, 1.12, T(g["rand_u_jitter"]), T(np.full(B, 0.3)), T(np.full(B, 1.0)))[2]
    _assert_same_bits(f"{name} z", N_(z), np.ascontiguousarray(g["st_z_coarse"][..., 0]))
