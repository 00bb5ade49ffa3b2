"""numpy restatement of the inverse-CDF resampling kernels (fenerf_amd/csrc/fenerf_composite.hip: resample_kernel<RAW, RS>, and the same
arithmetic fused into the coarse composite, fenerf_composite_ray.h), in the kernel's float32 operations step by step and in its order, so
that the library's result can be checked bit for bit on the CPU side.  The arithmetic is + - * / and comparisons only, the library is built
with -ffp-contract=off and without fast-math, and fp32 division is correctly rounded on both sides: every step below rounds as the kernel's.

One wave per ray, lane l of slot s holds pdf bin j = 64 s + l; RS slots per lane, chosen as launch_resample / launch_sample_pdf choose it."""
import numpy as np

F = np.float32
EPS = F(1e-5)


def _wave_sum(v):
    """wave_sum (fenerf_lane.h): the xor butterfly 32, 16, ... 1 over the last axis of 64 lanes; every lane ends with the same bits"""
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ o]
    return v


def _wave_scan_add(v):
    """wave_scan_add (fenerf_composite_ray.h): Hillis-Steele inclusive scan over 64 lanes, offsets 1, 2, ... 32"""
    v = v.copy()
    for o in (1, 2, 4, 8, 16, 32):
        t = v[..., :-o].copy()
        v[..., o:] = v[..., o:] + t
    return v


def _slots_resample(N):
    return 8 if N > 256 else (4 if N > 128 else 2)


def _slots_sample_pdf(K, NS):
    return 8 if (K > 255 or NS > 256) else (4 if (K > 127 or NS > 128) else 2)


def _inverse_cdf(bins, ww, u, RS):
    """bins [BR, K + 1] (s_bin), ww [BR, K] (the weights after their + 1e-5 additions), u [BR, NS] -> (samples [BR, NS], cdf [BR, K + 1])"""
    BR, K = ww.shape
    assert bins.shape == (BR, K + 1) and K + 1 <= 64 * RS and u.shape[1] <= 64 * RS and K >= 1
    lanes = np.zeros((BR, RS * 64), dtype=F)
    lanes[:, :K] = ww
    lanes = lanes.reshape(BR, RS, 64)                     # [ray, slot, lane]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        wsum = lanes[:, 0]
        for s in range(1, RS):                            # per-lane sum over the slots, in slot order
            wsum = wsum + lanes[:, s]
        tot = _wave_sum(wsum)                             # [BR, 64], the same value in every lane
        cdf = np.zeros((BR, RS * 64 + 1), dtype=F)        # cdf[0] = 0
        base = np.zeros((BR,), dtype=F)
        for s in range(RS):
            if 64 * s < K:
                inc = _wave_scan_add(lanes[:, s] / tot)
                cdf[:, 64 * s + 1:64 * s + 65] = inc if s == 0 else base[:, None] + inc
                base = inc[:, 63] if s == 0 else base + inc[:, 63]
        cdf = np.ascontiguousarray(cdf[:, :K + 1])        # the kernel stores (and reads) knots 0 .. K only
        inds = (cdf[:, None, :] < u[:, :, None]).sum(-1)  # searchsorted-left as a count over the K + 1 knots
        below = np.maximum(inds - 1, 0)
        above = np.minimum(inds, K)
        c0, c1 = np.take_along_axis(cdf, below, 1), np.take_along_axis(cdf, above, 1)
        b0, b1 = np.take_along_axis(bins, below, 1), np.take_along_axis(bins, above, 1)
        denom = c1 - c0
        denom = np.where(denom < EPS, F(1), denom)
        out = b0 + (u - c0) / denom * (b1 - b0)
    assert out.dtype == F and cdf.dtype == F
    return out, cdf


def resample(z_coarse, weights, u):
    """resample_kernel<false, RS> / the fused resample of composite_ray: z_coarse, weights, u [BR, N] (3 <= N <= 512) -> (fine z [BR, N],
    cdf [BR, N - 1]).  Bins are the midpoints of neighbouring coarse depths, their weights the interior coarse weights + 1e-5 + 1e-5."""
    z, w, u = (np.ascontiguousarray(a, dtype=F) for a in (z_coarse, weights, u))
    BR, N = z.shape
    assert w.shape == (BR, N) and u.shape == (BR, N) and 3 <= N <= 512
    with np.errstate(invalid="ignore", over="ignore"):
        ww = (w[:, 1:-1] + EPS) + EPS                     # two roundings
        bins = F(0.5) * (z[:, :-1] + z[:, 1:])
    return _inverse_cdf(bins, ww, u, _slots_resample(N))


def sample_pdf(bins, weights, u):
    """resample_kernel<true, RS>: bins [BR, K + 1], weights [BR, K], u [BR, NS] (1 <= K <= 511, 1 <= NS <= 512) -> (samples [BR, NS],
    cdf [BR, K + 1])"""
    b, w, u = (np.ascontiguousarray(a, dtype=F) for a in (bins, weights, u))
    BR, K = w.shape
    assert b.shape == (BR, K + 1) and u.shape[0] == BR and 1 <= K <= 511 and 1 <= u.shape[1] <= 512
    with np.errstate(invalid="ignore", over="ignore"):
        ww = w + EPS
    return _inverse_cdf(b, ww, u, _slots_sample_pdf(K, u.shape[1]))
