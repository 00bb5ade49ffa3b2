"""The three oracles on non-finite inputs against the reference's own answers (tests/golden/nonfinite_*.npz, recorded by
tools/make_golden.py::run_nonfinite from the reference's fancy_integration, sample_pdf, its cat / sort / gather merge and the SIREN modules'
forward and autograd with ONE NaN / +Inf / -Inf injected): the finite / non-finite mask EXACTLY, the finite values to the bounds of
tests/test_oracle_golden.py.  That is what lets tests/test_gpu_nonfinite.py use the oracles as the arbiter at shapes that have no fixture."""
import ast
import warnings

import numpy as np
import pytest
import torch

from conftest import load_golden, spec_from_golden
from fenerf_amd import procedural as proc
from oracle import fenerf_oracle as O
from oracle import fenerf_oracle_grad as OG
from oracle import fenerf_oracle_torch as OT

VALUES = {"nan": np.nan, "pinf": np.inf, "ninf": -np.inf}


def _same(tag, got, ref, atol, rtol=0.0):
    """the same elements finite, the finite ones within the bound, and a non-finite element of the same KIND (the oracles restate the
    reference's arithmetic op for op)"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin), (tag, "finite mask", int((~np.isfinite(got)).sum()), int((~fin).sum()))
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (tag, "NaN vs Inf")
    np.testing.assert_allclose(got[fin], ref[fin], atol=atol, rtol=rtol, err_msg=tag)
    return int((~fin).sum())


def _composite_cases():
    g = load_golden("nonfinite_composite")
    return g, [str(g[f"c{i}_id"]) for i in range(int(g["n_cases"]))]


_G, _IDS = _composite_cases()


@pytest.mark.parametrize("i", range(len(_IDS)), ids=_IDS)
def test_oracles_composite_nonfinite(i):
    g = _G
    kw = ast.literal_eval(str(g[f"c{i}_kw"]))
    rs, z, noise = g["base_rs"].copy(), g["base_z"].copy(), g["base_noise"].copy()
    what, idx, v = ast.literal_eval(str(g[f"c{i}_inj"]))
    {"rs": rs, "z": z, "noise": noise}[what][idx] = VALUES[v]
    assert (~np.isfinite(rs)).sum() + (~np.isfinite(z)).sum() + (~np.isfinite(noise)).sum() == 1
    ref = (g[f"c{i}_rgb"], g[f"c{i}_depth"], g[f"c{i}_third"])
    assert not np.isfinite(ref[0][0, 1]).all() or "pinf" in _IDS[i] or "ninf" in _IDS[i]     # the reference does not swallow a NaN
    for r in ref:                                                                             # and the other rays never see it
        assert np.isfinite(np.delete(r, 1, axis=1)).all()
    with np.errstate(all="ignore"):
        got = O.fancy_integration(rs, z, noise=noise, **kw)
    n = [_same(f"numpy {_IDS[i]} {k}", a, b, 3e-6) for k, a, b in zip(("rgb", "depth", "third"), got, ref)]
    got = OT.fancy_integration(torch.from_numpy(rs), torch.from_numpy(z), noise=torch.from_numpy(noise), **kw)
    for k, a, b in zip(("rgb", "depth", "third"), got, ref):
        _same(f"torch {_IDS[i]} {k}", a.numpy(), b, 3e-6)
    if "fill_mode" not in kw:      # the differentiable restatement (fp64; fill modes are not differentiated)
        t64 = lambda a: torch.tensor(a, dtype=torch.float64)
        rgb, depth, w = OG.composite(t64(rs[0]), t64(z[0, ..., 0]), t64(noise[0, ..., 0]), **kw)
        for k, a, b in zip(("rgb", "depth", "third"), (rgb, depth, w), ref):
            _same(f"grad {_IDS[i]} {k}", a.numpy().astype(np.float32).reshape(b.shape), b, 3e-6)
    print(f"[nonfinite-cpu] composite {_IDS[i]}: non-finite rgb/depth/weights elements {n}")


def test_oracles_merge_sort_and_sample_pdf_nonfinite():
    g = _G
    for j in range(int(g["n_merges"])):
        fine, coarse, zf, zc = (g[f"m{j}_{k}"] for k in ("fine", "coarse", "zf", "zc"))
        ao, az = O.merge_sorted(fine, coarse, zf, zc)
        assert np.array_equal(az, g[f"m{j}_all_z"], equal_nan=True)
        idx = np.argsort(np.concatenate([zf, zc], -2), axis=-2, kind="stable")
        assert np.array_equal(idx, g[f"m{j}_indices"])                          # NaN after +Inf, NaNs and ties in input order
        zz = g[f"m{j}_all_z"][0, 1, :, 0]
        k = int(np.isnan(zz).sum())
        assert (k == 0 or np.isnan(zz[-k:]).all()) and not np.isnan(zz[:len(zz) - k]).any()
        with np.errstate(all="ignore"):
            got = O.fancy_integration(ao, az, clamp_mode="relu")
        for k_, a, b in zip(("rgb", "depth", "third"), got, (g[f"m{j}_rgb"], g[f"m{j}_depth"], g[f"m{j}_third"])):
            _same(f"numpy merge {j} {k_}", a, b, 3e-6)
        t64 = lambda a: torch.tensor(a, dtype=torch.float64)
        rgb, depth, w = OG.merge_composite(t64(fine[0]), t64(coarse[0]), t64(zf[0, ..., 0]), t64(zc[0, ..., 0]), clamp_mode="relu")
        _same(f"grad merge {j} rgb", rgb.numpy().astype(np.float32), g[f"m{j}_rgb"][0], 3e-6)
        _same(f"grad merge {j} weights", w.numpy().astype(np.float32), g[f"m{j}_third"][0, ..., 0], 3e-6)
    for j in range(int(g["n_pdf"])):
        bins, w, u, ref = (g[f"p{j}_{k}"] for k in ("bins", "weights", "u", "samples"))
        assert not np.isfinite(ref[1]).any() and np.isfinite(np.delete(ref, 1, axis=0)).all()      # the whole ray, only that ray
        with np.errstate(all="ignore"):
            _same(f"numpy sample_pdf {j}", O.sample_pdf(bins, w, u), ref, 2e-6)
        _same(f"torch sample_pdf {j}", OT.sample_pdf(torch.from_numpy(bins), torch.from_numpy(w), torch.from_numpy(u)).numpy(), ref, 2e-6)


@pytest.mark.parametrize("kind", ["texture", "baseline", "spatial"])
def test_oracles_siren_nonfinite(kind):
    g = load_golden(f"nonfinite_siren_{kind}")
    spec = spec_from_golden(g)
    sd = proc.make_state_dict(spec, seed=int(g["meta_seed"]), sigma_gain=float(g["meta_sigma_gain"]))
    assert abs(proc.checksum(sd) - float(g["meta_weights_checksum"])) < 1e-9
    render = {k: v for k, v in sd.items() if "mapping_network" not in k}
    sig_tol = 1e-4 * max(1.0, float(g["meta_sigma_gain"]) / 20)
    for i in range(int(g["n_cases"])):
        cid = str(g[f"c{i}_id"])
        a = {k: g["base_" + k].copy() for k in ("points", "dirs", "loss_w", "freq_geo", "phase_geo", "freq_app", "phase_app")}
        what, idx, v = ast.literal_eval(str(g[f"c{i}_inj"]))
        a[what][idx] = VALUES[v]
        ref = g[f"c{i}_out"]
        if kind == "spatial":      # the single-latent oracles take the module's one concatenated FiLM tensor
            args = (np.concatenate([a["freq_geo"], a["freq_app"]], -1), np.concatenate([a["phase_geo"], a["phase_app"]], -1))
        else:
            args = (a["freq_geo"], a["phase_geo"], a["freq_app"], a["phase_app"])
        with np.errstate(all="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out = O.siren_forward(render, spec, a["points"], a["dirs"], *args)
        ot = OT.siren_forward(OT.state_to_torch(render), spec, torch.from_numpy(a["points"]), torch.from_numpy(a["dirs"]),
                              *(torch.from_numpy(x) for x in args)).numpy()
        for tag, got in (("numpy", out), ("torch", ot)):
            assert np.array_equal(np.isfinite(got), np.isfinite(ref)), (kind, cid, tag)
            fin = np.isfinite(ref)
            np.testing.assert_allclose(got[..., :-1][fin[..., :-1]], ref[..., :-1][fin[..., :-1]], atol=2e-5, rtol=1e-4)
            np.testing.assert_allclose(got[..., -1][fin[..., -1]], ref[..., -1][fin[..., -1]], atol=sig_tol, rtol=2e-4)
        # the differentiable restatement: forward mask, and per gradient tensor the finite mask of the reference's own autograd
        t64 = lambda x: torch.tensor(np.asarray(x), dtype=torch.float64)
        sd64 = {k: t64(v).requires_grad_(True) for k, v in render.items()}
        f64 = {k: t64(a[k]).requires_grad_(True) for k in ("freq_geo", "phase_geo", "freq_app", "phase_app")}
        o64 = OG.siren_forward(sd64, spec, t64(a["points"]), t64(a["dirs"]), f64["freq_geo"], f64["phase_geo"], f64["freq_app"], f64["phase_app"])
        assert np.array_equal(np.isfinite(o64.detach().numpy()), np.isfinite(ref)), (kind, cid, "grad oracle forward")
        (o64 * t64(a["loss_w"])).sum().backward()
        n_bad = 0
        for k, v in list(f64.items()) + list(sd64.items()):
            key = f"c{i}_grad_film_{k}" if k in f64 else f"c{i}_grad_{k}"
            if key not in g:        # weight gradients are recorded for the backward cases (phase-nan, grad-nan, grad-pinf)
                assert k in sd64 and cid not in ("phase-nan", "grad-nan", "grad-pinf")
                continue
            r = g[key]
            got = v.grad.numpy().astype(np.float32) if v.grad is not None else np.zeros_like(r)
            assert np.array_equal(np.isfinite(got), np.isfinite(r)), (kind, cid, k, int((~np.isfinite(got)).sum()), int((~np.isfinite(r)).sum()))
            fin = np.isfinite(r)
            if fin.any():
                assert np.abs(got[fin] - r[fin]).max() <= 1e-4 * max(1.0, np.abs(r[fin]).max()), (kind, cid, k)
            n_bad += int((~fin).sum())
        print(f"[nonfinite-cpu] {kind} {cid}: {int((~np.isfinite(ref)).sum())} non-finite outputs, {n_bad} non-finite gradient elements")


def test_bf16_backward_stream_keeps_a_nan_weight_a_nan():
    """The bf16 (hi, lo) halves of the backward chain stream are rounded by an integer add on the bit pattern: a NaN whose mantissa is all
    ones (0x7fffffff, 0xffffffff) carried into the sign / out of the word and became -0 / +0 in BOTH halves -- a NaN weight that the
    backward never saw.  Every half that a NaN weight feeds must be a NaN.  (Host code of the built libfenerf_hip.so, like the pack-layout
    tests: no GPU, but the library must have been built.)"""
    from fenerf_amd import _lib
    spec = proc.model_spec("texture", hidden_dim=32, grid_size=4, z_dim=8)
    sd = proc.make_state_dict(spec, seed=4, sigma_gain=30.0, with_mapping=False)
    clean = _lib.pack_backward_host(sd, spec, "f16x3")
    for bits in (0x7fc00000, 0x7fffffff, 0xffffffff, 0xffc00001):
        sd2 = {k: v.copy() for k, v in sd.items()}
        sd2["network.3.layer.weight"].view(np.uint32)[2, 5] = bits
        blob = _lib.pack_backward_host(sd2, spec, "f16x3")
        assert blob.shape == clean.shape
        h, h0 = blob.view(np.uint16), clean.view(np.uint16)
        changed = np.flatnonzero(h != h0)
        is_nan = ((h[changed] & 0x7f80) == 0x7f80) & ((h[changed] & 0x007f) != 0)
        assert changed.size >= 2 and is_nan.all(), (hex(bits), changed.size, [hex(x) for x in h[changed][:8]])
