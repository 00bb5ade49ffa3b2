"""Deterministic inputs of the ray-tail tests (tests/test_ray_tail_cpu.py, tests/test_gpu_ray_tail.py): the CPU and the GPU tests build
their arrays HERE, so both see the same bits.  A plain helper module -- numpy only, plus the project's own numpy emulation and oracle."""
import functools
import itertools
import math

import numpy as np

from fenerf_amd import resample_emulation as RE
from oracle import fenerf_oracle as O

F = np.float32
EPS24 = 2.0 ** -24

# ---------------------------------------------------------------------------------------------------
# inverse-CDF resampling
# ---------------------------------------------------------------------------------------------------
RESAMPLE_N = [3, 4, 5, 64, 65, 66, 67, 127, 128, 129, 130, 131, 255, 256, 257, 258, 259, 511, 512]
SAMPLE_PDF_SHAPES = [(1, 1), (1, 130), (63, 64), (64, 64), (65, 3), (127, 128), (127, 129), (128, 128), (255, 256), (255, 257), (256, 5),
                     (5, 512), (511, 512)]
RESAMPLE_RAYS = 11          # 4 rays per workgroup: the last one is ragged
EXACT_DRAWS = np.array([0.0, 1.0, 1.0 - 2.0 ** -24, 2.0 ** -149], dtype=F)
assert EXACT_DRAWS[2] < 1 and EXACT_DRAWS[3] > 0


# The oracle's `denom < 1e-5 -> 1` is a jump of the inverse cdf in the WEIGHTS: a bin whose fp64 mass is within rounding of 1e-5 is clamped
# by one arithmetic and not by the other, and no backward error in u describes that.  So no bin of a case may sit there.  The fp32 mass of
# a bin is the difference of two neighbouring knots; what the two do not share is the last scan level that separates them and the addition
# of the slot base, each rounded to half an ulp of a value below 1 (2^-25): 4 * 2^-25 = 2^-23.  A cap on the inputs, taken on the fp64
# reference alone (tests/test_ray_tail_cpu.py asserts it); random bins are moved twice as far away, the EMPTY bins of the mass-0.98 ray
# stay where that mass puts them: 1.5e-7 .. 2e-7 above the clamp with sample_pdf's one + 1e-5.
CLAMP_MARGIN = 2.0 ** -23


def pdf64(w_bins, eps_total):
    """fp64 mass of every pdf bin [BR, K] from the fp32 weights of the bins; eps_total: 1e-5 (sample_pdf) or 2e-5 (resample)"""
    ww = np.asarray(w_bins, dtype=np.float64) + eps_total
    return ww / ww.sum(-1, keepdims=True)


def _clear_of_clamp(w, eps_total):
    for _ in range(200):
        bad = (np.abs(pdf64(w, eps_total) - 1e-5) <= 2 * CLAMP_MARGIN) & (w > 0)
        if not bad.any():
            return w
        w[bad] *= F(1.25)
    raise AssertionError("could not move the bins away from the clamp")


def _pdf_rays(rng, K, NS, eps_total):
    """-> weights [11, K] of the K pdf bins, depths of the knots [11, K + 1], draws [11, NS]; one ray of each kind where K allows"""
    BR = RESAMPLE_RAYS
    w = rng.random((BR, K)).astype(F) ** 4                                 # 0: random w^4 (rays of a kind that K does not allow stay so)
    knots = np.sort(rng.uniform(0.88, 1.12, (BR, K + 1)).astype(F), axis=1)
    u = rng.random((BR, NS)).astype(F)
    w[1] = 0                                                               # 1: all-zero weights
    w[2] = 0
    w[2, K // 2] = F(0.37)                                                 # 2: one non-zero weight
    if K > 66:
        w[3, 60:67] = 0                                                    # 3: an empty stretch straddling bins 63 / 64
    for ray, mass in ((4, 0.05), (5, 0.98), (6, 40.0)):                    # 4-6: empty bins above, at and below the 1e-5 clamp
        if K >= 3:
            w[ray, rng.random(K) < 0.35] = 0
        if w[ray].sum() == 0:
            w[ray, 0] = 1
        w[ray] = (w[ray].astype(np.float64) * (mass / w[ray].astype(np.float64).sum())).astype(F)
    if K >= 2:
        knots[7, 1::2] = knots[7, 0:-1:2][:knots[7, 1::2].size]            # 7: equal neighbouring depths (zero-width bins)
    u[8, :min(4, NS)] = EXACT_DRAWS[:min(4, NS)]                           # 8: u = 0, 1, 1 - 2^-24, 2^-149
    if NS > 8:
        u[8, -4:] = EXACT_DRAWS[::-1]                                      #    and in the last slot too
    return _clear_of_clamp(w, eps_total), knots, u


def _knot_draws(u, cdf):
    """ray 9: the draws are the emulation's own cdf knots (searchsorted-left on ties), cycled over the NS draws"""
    NS = u.shape[1]
    u[9] = cdf[9][np.arange(NS) % cdf.shape[1]]
    return u


@functools.lru_cache(maxsize=None)
def resample_case(N):
    """-> z_coarse, weights, u [11, N] (float32)"""
    rng = np.random.default_rng(1000 + N)
    K = N - 2
    wk, _, u = _pdf_rays(rng, K, N, 2e-5)
    z = np.sort(rng.uniform(0.88, 1.12, (RESAMPLE_RAYS, N)).astype(F), axis=1)
    if N >= 4:                                                             # 7: three equal depths in a row: two equal midpoints, a zero-width bin
        z[7] = np.repeat(z[7, :(N + 2) // 3], 3)[:N]
    w = rng.random((RESAMPLE_RAYS, N)).astype(F)                           # the first and the last coarse weight are not part of the pdf
    w[:, 1:-1] = wk
    _, cdf = RE.resample(z, w, u)
    u = _knot_draws(u, cdf)
    for a in (z, w, u):
        a.setflags(write=False)
    return z, w, u


@functools.lru_cache(maxsize=None)
def sample_pdf_case(K, NS):
    """-> bins [11, K + 1], weights [11, K], u [11, NS] (float32)"""
    rng = np.random.default_rng(2000 + 1000 * K + NS)
    w, bins, u = _pdf_rays(rng, K, NS, 1e-5)
    _, cdf = RE.sample_pdf(bins, w, u)
    u = _knot_draws(u, cdf)
    for a in (bins, w, u):
        a.setflags(write=False)
    return bins, w, u


def resample_f64(z, w, u):
    """the fp64 oracle on the fp32 inputs, u in float64 (so that u +- delta is representable)"""
    BR, N = z.shape
    return O.fine_z_from_coarse(w.astype(np.float64).reshape(1, BR, N, 1), z.astype(np.float64).reshape(1, BR, N, 1),
                                np.asarray(u, dtype=np.float64)).reshape(BR, N)


def sample_pdf_f64(bins, w, u):
    return O.sample_pdf(bins.astype(np.float64), w.astype(np.float64), np.asarray(u, dtype=np.float64))


DELTA = 2.0 ** -20          # 16 roundings of quantities <= 1: 6 scan levels, <= 7 slot bases, the division, u - c0 and the compare
DELTA_LADDER = [2.0 ** -k for k in range(26, 9, -1)]


def bracket_ok(f64, got, u, delta, zmax):
    """F64(u - delta) - tau <= got <= F64(u + delta) + tau on every sample (the inverse cdf is monotone in u, not continuous at the clamp)"""
    tau = 4 * EPS24 * zmax
    u = u.astype(np.float64)
    g = got.astype(np.float64)
    return bool(((f64(u - delta) - tau <= g) & (g <= f64(u + delta) + tau)).all())


def needed_delta(f64, got, u, zmax):
    """the smallest delta on the ladder 2^-26 ... 2^-10 for which the bracket holds on every sample (inf: none)"""
    for d in DELTA_LADDER:
        if bracket_ok(f64, got, u, d, zmax):
            return d
    return math.inf


# ---------------------------------------------------------------------------------------------------
# composite
# ---------------------------------------------------------------------------------------------------
COMPOSITE_M = [2, 3, 63, 64, 65, 127, 128, 129, 191, 192, 193, 256, 257, 512, 513, 1023, 1024]
COMPOSITE_C = [2, 4, 22, 33, 34, 36]
# (clamp_mode, noise_std, last_back, white_back, black_back)
FLAG_SETS = [(c, ns, lb, bk == "white", bk == "black") for c, ns, lb, bk in
             itertools.product(("relu", "softplus"), (0.0, 0.5, -0.3), (False, True), (None, "white", "black"))]
FULL_PRODUCT_M = [65, 130]
CEILING = {"rgb": 2e-5, "depth": 2e-5, "weights": 1e-5, "wsum": 1e-5}      # what the suite already holds these outputs to


def flags_id(f):
    return f"{f[0]}-n{f[1]}-{'lb' if f[2] else 'nolb'}-{'white' if f[3] else 'black' if f[4] else 'plain'}"


def composite_rotation():
    """each M with one C and one flag set in rotation: every C at least twice and at least once with M > 64; the flag sets advance by 7
    (coprime to 36), so neighbouring M differ in every flag.  (Every flag set appears twice with M > 64 in the full product at M = 65, 130.)"""
    return [(M, COMPOSITE_C[i % len(COMPOSITE_C)], FLAG_SETS[(7 * i + 3) % len(FLAG_SETS)]) for i, M in enumerate(COMPOSITE_M)]


@functools.lru_cache(maxsize=None)
def composite_case(M, C, BR=9, seed=0):
    """-> rows [BR, M, C] (sigma ~ 30 N(0,1) last), z [BR, M] ascending, noise [BR, M] (un-scaled N(0,1))"""
    rng = np.random.default_rng(3000 + 7 * M + C + seed)
    rs = rng.normal(size=(BR, M, C)).astype(F)
    rs[..., -1] *= 30
    z = np.sort(rng.uniform(0.88, 1.12, (BR, M)).astype(F), axis=1)
    noise = rng.normal(size=(BR, M)).astype(F)
    for a in (rs, z, noise):
        a.setflags(write=False)
    return rs, z, noise


def graded_case(M, C, BR=16):
    """fill cases: density scale geomspace(0.05, 60, BR) per ray, a negative sigma on the last sample (its delta is 1e10): weights_sum from
    0.009 to 1.0 with nothing near the 0.9 threshold"""
    return _graded_case(M, C, BR)


@functools.lru_cache(maxsize=None)
def _graded_case(M, C, BR):
    rng = np.random.default_rng(4000 + 7 * M + C)
    rs = rng.normal(size=(BR, M, C)).astype(F)
    rs[..., -1] = np.abs(rng.normal(size=(BR, M))).astype(F) * np.geomspace(0.05, 60, BR).astype(F)[:, None]
    rs[:, -1, -1] = F(-1)
    z = np.sort(rng.uniform(0.88, 1.12, (BR, M)).astype(F), axis=1)
    for a in (rs, z):
        a.setflags(write=False)
    return rs, z


FILL_M = [12, 65, 130, 513]
# (fill_mode, fill_color, C or None for the case's own)
FILL_MODES = [("weight", "black", None)] + [("seg_padding_background", c, None) for c in ("white", "black", "grey", "light_grey", "magenta")] + \
             [("eval_seg_padding_background", "grey", None), ("eval_white_back", "black", 4)]


def fill_channels(M):
    return 36 if M in (65, 130) else 22


def oracle_composite(rs, z, noise, flags, dtype, fill_mode=None, fill_color="black"):
    """O.fancy_integration in `dtype` on the fp32 inputs (the noise un-scaled, as the oracle expects; noise_std the fp32 value the library is
    handed) -> dict(rgb [BR, C'], depth [BR], weights [BR, M], wsum [BR])"""
    clamp, ns, lb, wb, bb = flags
    dt = np.dtype(dtype)
    rows, zz = rs.astype(dt)[None], z.astype(dt)[None, ..., None]
    nz = noise.astype(dt)[None, ..., None] if (noise is not None and ns != 0) else None
    kw = dict(noise=nz, noise_std=float(F(ns)), last_back=lb, white_back=wb, black_back=bb, clamp_mode=clamp)
    rgb, depth, w = O.fancy_integration(rows, zz, **kw)
    w0 = w                                    # weights_sum is taken BEFORE the last_back adjustment (volumetric_rendering.py:38-41)
    if lb:
        w0 = O.fancy_integration(rows, zz, **dict(kw, last_back=False))[2]
    if fill_mode is not None:
        rgb = O.fancy_integration(rows, zz, fill_mode=fill_mode, fill_color=fill_color, **kw)[0]
    assert rgb.dtype == dt and w.dtype == dt
    return dict(rgb=rgb[0], depth=depth[0, ..., 0], weights=w[0, ..., 0], wsum=w0[0, ..., 0].sum(-1, dtype=dt))


def alpha_arguments(rs, z, noise, flags):
    """the fp64 arguments delta * act(sigma + noise) of the alpha exponentials [BR, M]"""
    clamp, ns, _, _, _ = flags
    x = rs[..., -1].astype(np.float64) + (noise.astype(np.float64) * float(F(ns)) if noise is not None else 0.0)
    act = O._softplus(x) if clamp == "softplus" else np.maximum(x, 0)
    delta = np.concatenate([np.diff(z.astype(np.float64), axis=-1), np.full(z.shape[:-1] + (1,), 1e10)], -1)
    return delta * act


def value_bound(name, e32, ref):
    """4 e32 + 8 * 2^-24 * max(1, max|ref|), never above the ceiling the suite already uses.  e32: the fp32 numpy oracle's own max error on
    the same inputs; the factor 4: scan-tree product order, device expf / log1pf, the two-lane channel sum."""
    ref = np.asarray(ref)
    scale = max(1.0, float(np.abs(ref).max())) if ref.size else 1.0
    return min(4 * e32 + 8 * EPS24 * scale, CEILING[name])


def max_err(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max()) if ref.size else 0.0


# ---------------------------------------------------------------------------------------------------
# merge composite
# ---------------------------------------------------------------------------------------------------
MERGE_N = [2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 256, 257, 511, 512]
MERGE_RAYS = 7
MERGE_FLAGS = [("relu", 0.4, False, False, False), ("softplus", 0.0, True, False, False), "graded"]


def merge_rotation():
    """(N, C, flag set): the three flag sets in rotation, C = 22, and one more case with C = 36"""
    return [(N, 22, i % 3) for i, N in enumerate(MERGE_N)] + [(65, 36, 0)]


def _tied_ray(rng, N):
    """2 N depths, one fine and one coarse sample on the SAME depth at sorted positions 63 / 64 and 127 / 128 (where 2 N reaches them)"""
    ties = [p for p in (63, 127) if p + 1 < 2 * N]
    vals = np.unique(rng.uniform(0.88, 1.12, 4 * N).astype(F))[:2 * N - len(ties)]
    assert vals.size == 2 * N - len(ties)
    merged = list(vals)
    for p in ties:                      # duplicate the value at sorted position p: the pair sits at p, p + 1
        merged.insert(p + 1, merged[p])
    merged = np.array(merged, dtype=F)
    assert all(merged[p] == merged[p + 1] for p in ties) and (np.diff(merged) >= 0).all()
    to_fine = np.zeros(2 * N, dtype=bool)
    free = [i for i in range(2 * N) if all(i not in (p, p + 1) for p in ties)]
    for p in ties:
        to_fine[p] = True
    to_fine[rng.permutation(free)[:N - len(ties)]] = True
    return merged[to_fine], merged[~to_fine]


@functools.lru_cache(maxsize=None)
def merge_case(N, C, flag_index):
    """-> fine, coarse [7, N, C], z_fine [7, N] (unsorted, as sample_pdf leaves it), z_coarse [7, N] ascending, noise [7, 2 N]"""
    rng = np.random.default_rng(5000 + 11 * N + C + flag_index)
    BR = MERGE_RAYS
    fine = rng.normal(size=(BR, N, C)).astype(F)
    coarse = rng.normal(size=(BR, N, C)).astype(F)
    zc = np.sort(rng.uniform(0.88, 1.12, (BR, N)).astype(F), axis=1)
    zf = rng.uniform(0.88, 1.12, (BR, N)).astype(F)                        # 0: random
    zf[1] = zc[1]                                                          # 1: every fine depth copied from a coarse one
    if N > 32:
        f, c = _tied_ray(rng, N)                                           # 2: ties on sorted positions 63 / 64 (and 127 / 128)
        zf[2], zc[2] = f, c
    zf[3] = zc[3] = F(1.0)                                                 # 3: all depths equal
    zf[4] = rng.uniform(0.5, 0.87, N).astype(F)                            # 4: fine entirely before coarse
    zf[5] = rng.uniform(1.13, 1.5, N).astype(F)                            # 5: fine entirely after coarse
    zf[6, ::3] = zc[6, ::3]                                                # 6: every third fine depth copied from a coarse one
    for r in range(BR):                                                    # unsorted, ties included
        zf[r] = zf[r][rng.permutation(N)]
    noise = rng.normal(size=(BR, 2 * N)).astype(F)
    if MERGE_FLAGS[flag_index] == "graded":
        scale = np.geomspace(0.05, 60, BR).astype(F)[:, None]
        fine[..., -1] = np.abs(rng.normal(size=(BR, N))).astype(F) * scale
        coarse[..., -1] = np.abs(rng.normal(size=(BR, N))).astype(F) * scale
        last = np.argsort(np.concatenate([zf, zc], 1), axis=1, kind="stable")[:, -1]      # the last sorted sample: its delta is 1e10
        for r, s in enumerate(last):
            (fine if s < N else coarse)[r, s % N, -1] = F(-1)
    else:
        fine[..., -1] *= 30
        coarse[..., -1] *= 30
    for a in (fine, coarse, zf, zc, noise):
        a.setflags(write=False)
    return fine, coarse, zf, zc, noise


def merge_flags(flag_index):
    """-> (flags, fill_mode, fill_color)"""
    f = MERGE_FLAGS[flag_index]
    if f == "graded":
        return ("relu", 0.0, False, False, False), "seg_padding_background", "grey"
    return f, None, "black"


def oracle_merge(fine, coarse, zf, zc, noise, flags, dtype, fill_mode=None, fill_color="black"):
    """O.merge_sorted then O.fancy_integration in `dtype` -> the dict of oracle_composite plus z_sorted [BR, 2 N]"""
    dt = np.dtype(dtype)
    rows, z = O.merge_sorted(fine.astype(dt)[None], coarse.astype(dt)[None], zf.astype(dt)[None, ..., None], zc.astype(dt)[None, ..., None])
    out = oracle_composite(rows[0], z[0, ..., 0], noise, flags, dtype, fill_mode, fill_color)
    out["z_sorted"] = z[0, ..., 0]
    return out


# ---------------------------------------------------------------------------------------------------
# ray setup
# ---------------------------------------------------------------------------------------------------
RAY_PHI = np.array([-0.2, math.pi / 2, math.pi + 1], dtype=F)              # below the pitch clamp, inside, above it
RAY_THETA = np.array([-7.0, 0.3, 2 * math.pi + 1], dtype=F)
# (S, N, fov, (ray_start, ray_end)): every S, N, fov and depth range, a small rotation
RAY_SETUP_CASES = [(1, 2, 12, (0.88, 1.12)), (2, 3, 30, (0.1, 5.0)), (3, 12, 30, (0.88, 1.12)), (5, 13, 12, (0.1, 5.0)),
                   (16, 3, 12, (0.88, 1.12)), (17, 2, 30, (0.1, 5.0)), (17, 13, 12, (0.88, 1.12)), (3, 12, 12, (0.1, 5.0))]


def ray_setup_jitter(S, N):
    return np.random.default_rng(6000 + 31 * S + N).random((3, S * S, N, 1)).astype(F)


def clamped_pitch(phi):
    """torch.clamp(phi, 1e-5, pi - 1e-5) on a float32 tensor: the bounds are rounded to float32, the comparison is in float32"""
    return np.clip(np.asarray(phi, dtype=F), F(1e-5), F(math.pi - 1e-5))


def oracle_ray_setup(S, N, fov, ray_range, u_jitter, theta, pitch, dtype):
    """The oracle's get_initial_rays_trig -> transform_sampled_points in `dtype`, fed the ALREADY CLAMPED float32 pitch.  Stated through the
    oracle's own steps (perturb_points, normalize_vecs, create_cam2world_matrix) without camera_origin's second clamp: at the `dtype`
    rounding of pi - 1e-5 that clamp would move the float32 pitch again, by 1e-7, which is 1 % of sin(pitch) there and the test's own
    error.  -> origins [B, R, 3], dirs [B, R, 3], z [B, R, N]"""
    dt = np.dtype(dtype).type
    B = len(theta)
    pts, z, d = O.get_initial_rays_trig(B, N, fov, (S, S), float(F(ray_range[0])), float(F(ray_range[1])), dtype=dt)   # the floats the library gets
    _, z = O.perturb_points(pts, z, d, np.asarray(u_jitter).astype(dt))
    th, ph = np.asarray(theta).astype(dt).reshape(B, 1), np.asarray(pitch).astype(dt).reshape(B, 1)
    o = np.concatenate([np.sin(ph) * np.cos(th), np.cos(ph), np.sin(ph) * np.sin(th)], -1).astype(dt)      # camera_origin, r = 1
    c2w = O.create_cam2world_matrix(O.normalize_vecs(-o), o)
    dirs = np.einsum("nij,npj->npi", c2w[:, :3, :3], d)
    origins = np.broadcast_to(o[:, None, :], dirs.shape)
    assert dirs.dtype == dt and z.dtype == dt and o.dtype == dt
    return origins, dirs, z[..., 0]
