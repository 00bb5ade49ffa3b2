"""The ray tail on a machine without a GPU: (a) the numpy emulation of the resampling kernels (fenerf_amd/resample_emulation.py, which
tests/test_gpu_ray_tail.py holds the kernels to bit for bit) against the fp64 oracle, as a backward-error bracket on EVERY sample;
(b) the conditions that the GPU cases of tests/ray_tail_cases.py rely on, established on the fp64 reference alone."""
import functools
import math

import numpy as np
import pytest

import ray_tail_cases as RC
from conftest import load_golden
from fenerf_amd import resample_emulation as RE
from oracle import fenerf_oracle as O


def _show(d):
    return f"2^{int(math.log2(d))}" if math.isfinite(d) else "none on the ladder"


@functools.lru_cache(maxsize=None)
def _resample(N):
    """-> (tag, fp64 oracle as a function of u, emulation, fp32 oracle, u, max|z|)"""
    z, w, u = RC.resample_case(N)
    emu, cdf = RE.resample(z, w, u)
    assert cdf.shape == (RC.RESAMPLE_RAYS, N - 1) and (cdf[:, 0] == 0).all() and (np.diff(cdf, axis=1) >= 0).all()
    o32 = O.fine_z_from_coarse(w.reshape(1, -1, N, 1), z.reshape(1, -1, N, 1), u).reshape(-1, N)
    return f"resample N={N}", lambda uu: RC.resample_f64(z, w, uu), emu, o32, u, float(np.abs(z).max())


@functools.lru_cache(maxsize=None)
def _sample_pdf(K, NS):
    bins, w, u = RC.sample_pdf_case(K, NS)
    emu, cdf = RE.sample_pdf(bins, w, u)
    assert cdf.shape == (RC.RESAMPLE_RAYS, K + 1) and (cdf[:, 0] == 0).all() and (np.diff(cdf, axis=1) >= 0).all()
    return f"sample_pdf K={K} NS={NS}", lambda uu: RC.sample_pdf_f64(bins, w, uu), emu, O.sample_pdf(bins, w, u), u, float(np.abs(bins).max())


def _assert_bracket(tag, f64, emu, o32, u, zmax):
    """delta = 2^-20, tau = 4 * 2^-24 * max|z|, no sample left out"""
    assert emu.dtype == np.float32 and emu.shape == u.shape and np.isfinite(emu).all()
    assert RC.bracket_ok(f64, emu, u, RC.DELTA, zmax), f"{tag}: the emulation leaves the fp64 bracket at delta = 2^-20"


@pytest.mark.parametrize("N", RC.RESAMPLE_N)
def test_resample_emulation_within_fp64_bracket(N):
    _assert_bracket(*_resample(N))


@pytest.mark.parametrize("K,NS", RC.SAMPLE_PDF_SHAPES)
def test_sample_pdf_emulation_within_fp64_bracket(K, NS):
    _assert_bracket(*_sample_pdf(K, NS))


def test_emulation_needs_no_wider_bracket_than_the_fp32_oracle():
    """The smallest delta on the ladder 2^-26 ... 2^-10 with which every sample of every case is inside the fp64 bracket: the emulation's
    (the kernel's scan tree) is no worse than the fp32 oracle's (sequential cumsum).  Over all cases, not case by case: on a single ray
    either order of summation can be the luckier one by a rung."""
    worst = {"emulation": 0.0, "fp32 oracle": 0.0}
    for case in [_resample(N) for N in RC.RESAMPLE_N] + [_sample_pdf(K, NS) for K, NS in RC.SAMPLE_PDF_SHAPES]:
        tag, f64, emu, o32, u, zmax = case
        d_emu, d_o32 = RC.needed_delta(f64, emu, u, zmax), RC.needed_delta(f64, o32, u, zmax)
        print(f"[ray-tail] {tag}: smallest delta: emulation {_show(d_emu)}, fp32 oracle {_show(d_o32)}")
        worst["emulation"], worst["fp32 oracle"] = max(worst["emulation"], d_emu), max(worst["fp32 oracle"], d_o32)
    print(f"[ray-tail] over all cases: emulation {_show(worst['emulation'])} = {worst['emulation']:.3e}, "
          f"fp32 oracle {_show(worst['fp32 oracle'])} = {worst['fp32 oracle']:.3e}")
    assert worst["emulation"] <= RC.DELTA and worst["emulation"] <= worst["fp32 oracle"]


def test_resample_cases_hold_what_they_claim():
    """the ray kinds of the cases are what the GPU test says they are"""
    for N in RC.RESAMPLE_N:
        z, w, u = RC.resample_case(N)
        _, cdf = RE.resample(z, w, u)
        assert (np.diff(z, axis=1) >= 0).all() and (w >= 0).all() and (u >= 0).all() and (np.delete(u, 9, 0) <= 1).all()
        assert (np.abs(RC.pdf64(w[:, 1:-1], 2e-5) - 1e-5) > RC.CLAMP_MARGIN).all()      # no bin within rounding of the clamp (fp64 alone)
        assert (w[1, 1:-1] == 0).all() and (w[2, 1:-1] != 0).sum() == 1
        assert np.isin(u[9], cdf[9]).all()                                          # draws ON the emulation's knots
        if N >= 6:
            assert set(RC.EXACT_DRAWS.tolist()) <= set(u[8].tolist())
        if N >= 7:
            mid = np.float32(0.5) * (z[7, :-1] + z[7, 1:])
            assert (np.diff(mid) == 0).any()                                        # zero-width bins
        if N > 68:
            assert (w[3, 61:68] == 0).all()                                         # pdf bins 60 .. 66 are coarse weights 61 .. 67
            gaps = np.diff(cdf, axis=1)
            assert (gaps[4][w[4, 1:-1] == 0] > 1e-5).all() and (gaps[6][w[6, 1:-1] == 0] < 1e-5).all()   # above / below the clamp
    for K, NS in RC.SAMPLE_PDF_SHAPES:
        bins, w, u = RC.sample_pdf_case(K, NS)
        _, cdf = RE.sample_pdf(bins, w, u)
        assert np.isin(u[9], cdf[9]).all() and (w[1] == 0).all()
        assert (np.abs(RC.pdf64(w, 1e-5) - 1e-5) > RC.CLAMP_MARGIN).all()
        if K >= 63:                                                                 # the mass-0.98 ray: its empty bins ARE at the clamp
            assert (w[5] == 0).any() and np.abs(RC.pdf64(w, 1e-5)[5][w[5] == 0] - 1e-5).max() < 2.5e-7
        if K >= 2:
            assert (np.diff(bins[7]) == 0).any()


def test_emulation_slot_counts_follow_the_launchers():
    """launch_resample: N > 256 -> 8, N > 128 -> 4, else 2 slots; launch_sample_pdf: K > 255 or NS > 256 -> 8, K > 127 or NS > 128 -> 4"""
    assert [RE._slots_resample(n) for n in (3, 128, 129, 256, 257, 512)] == [2, 2, 4, 4, 8, 8]
    assert [RE._slots_sample_pdf(k, ns) for k, ns in ((1, 1), (127, 128), (127, 129), (128, 128), (255, 256), (255, 257), (256, 5), (5, 512))] \
        == [2, 2, 4, 4, 4, 8, 8, 8]


def test_fill_cases_are_clear_of_the_threshold():
    """every ray of a fill case has |wsum64 - 0.9| > 1e-4, at least 3 rays on each side: the fill decision of the kernel's fp32 weights_sum
    (error <= 1e-5) must then equal fp64's on ALL rays -- a cap on the inputs, established on the reference alone"""
    flags = ("relu", 0.0, False, False, False)
    for M in RC.FILL_M:
        for C in {RC.fill_channels(M), 4}:
            rs, z = RC.graded_case(M, C)
            ws = RC.oracle_composite(rs, z, None, flags, np.float64)["wsum"]
            print(f"[ray-tail] fill case M={M} C={C}: wsum64 {ws.min():.4f} .. {ws.max():.4f}, nearest to 0.9: {np.abs(ws - 0.9).min():.2e}")
            assert (np.abs(ws - 0.9) > 1e-4).all() and (ws < 0.9).sum() >= 3 and (ws > 0.9).sum() >= 3
    for N, C, fi in RC.merge_rotation():
        if RC.MERGE_FLAGS[fi] == "graded":
            f, fill_mode, fill_color = RC.merge_flags(fi)
            ws = RC.oracle_merge(*RC.merge_case(N, C, fi), f, np.float64)["wsum"]
            assert (np.abs(ws - 0.9) > 1e-4).all() and (ws < 0.9).any() and (ws > 0.9).any(), (N, ws)


def test_composite_value_cases_do_not_overflow():
    """no fp64 argument of an alpha exponential overflows (nor would its fp32 rounding): delta * act is finite and below FLT_MAX"""
    cases = RC.composite_rotation() + [(M, 36, f) for M in RC.FULL_PRODUCT_M for f in RC.FLAG_SETS]
    for M, C, flags in cases:
        rs, z, noise = RC.composite_case(M, C)
        a = RC.alpha_arguments(rs, z, noise, flags)
        assert np.isfinite(a).all() and (a >= 0).all() and a.max() < 3e38, (M, C, flags)
    rot = RC.composite_rotation()
    assert {c for _, c, _ in rot} == set(RC.COMPOSITE_C)
    for C in RC.COMPOSITE_C:
        assert sum(1 for M, c, _ in rot if c == C) >= 2 and any(M > 64 for M, c, _ in rot if c == C)


def test_merge_cases_hold_what_they_claim():
    for N, C, fi in RC.merge_rotation():
        fine, coarse, zf, zc, noise = RC.merge_case(N, C, fi)
        allz = np.concatenate([zf, zc], 1)
        zs = np.sort(allz, axis=1)
        assert (np.diff(zc, axis=1) >= 0).all()
        assert np.isin(zf[1], zc[1]).all() and (allz[3] == allz[3, 0]).all()
        assert zf[4].max() < zc[4].min() and zf[5].min() > zc[5].max()
        if N > 1:
            assert (np.diff(zf[0]) < 0).any()                                       # unsorted, as sample_pdf leaves it
        for p in (63, 127):
            if p + 1 < 2 * N and N > 32:
                assert zs[2, p] == zs[2, p + 1] and np.isin(zs[2, p], zf[2]) and np.isin(zs[2, p], zc[2])
                assert (zs[2] == zs[2, p]).sum() == 2


@pytest.mark.parametrize("name", ["tiny_texture_fwd", "h256_texture_16x16_n24_trained"])
def test_oracle_depths_are_the_references_bits(name):
    """torch.linspace rounds start + step * i once (a fused multiply-add): the jittered depths the reference recorded are reproduced bit for
    bit by the fp32 oracle's depths, which the ray-setup kernel is held to.  With a separately rounded product, sample 9 of 24 is one ulp off."""
    g = load_golden(name)
    z, u = g["st_z_coarse"], g["rand_u_jitter"]
    B, R, N = z.shape[:3]
    S = int(round(math.sqrt(R)))
    pts, z0, d = O.get_initial_rays_trig(B, N, 12, (S, S), 0.88, 1.12)
    _, want = O.perturb_points(pts, z0, d, u)
    assert want.dtype == np.float32 and np.array_equal(np.ascontiguousarray(want).view(np.uint32), np.ascontiguousarray(z).view(np.uint32))


def test_ray_setup_pitch_clamp_is_float32():
    """the pitch the GPU test feeds the fp64 oracle: clamped in float32, both ends of the clamp reached, the middle untouched"""
    p = RC.clamped_pitch(RC.RAY_PHI)
    assert p.dtype == np.float32 and p[0] == np.float32(1e-5) and p[1] == RC.RAY_PHI[1] and p[2] == np.float32(math.pi - 1e-5)
    for S, N, fov, rng_ in RC.RAY_SETUP_CASES:
        u = RC.ray_setup_jitter(S, N)
        o64, d64, z64 = RC.oracle_ray_setup(S, N, fov, rng_, u, RC.RAY_THETA, p, np.float64)
        o32, d32, z32 = RC.oracle_ray_setup(S, N, fov, rng_, u, RC.RAY_THETA, p, np.float32)
        assert o32.dtype == np.float32 and o64.shape == (3, S * S, 3) and z64.shape == (3, S * S, N)
        np.testing.assert_allclose(np.linalg.norm(d64, axis=-1), 1, atol=1e-12)
        np.testing.assert_allclose(np.linalg.norm(o64, axis=-1), 1, atol=1e-12)
        for a, b in ((o32, o64), (d32, d64), (z32, z64)):
            assert RC.max_err(a, b) < 1e-5
