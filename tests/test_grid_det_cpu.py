"""CPU side of the deterministic feature-grid gradient: the numpy restatement of fenerf_grid_backward_det (fenerf_amd/grid_det_emulation.py)
against an fp64 np.add.at of the same transpose, within the resolution it states; the switch that selects the route; the C-ABI's new names."""
import os

import numpy as np
import pytest
import torch

from fenerf_amd import _lib
from fenerf_amd import grid_det_emulation as E
from fenerf_amd.siren import autograd as SA
from fenerf_amd.siren import siren as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("scale,hot", [(1.0, False), (1.0, True), (1e-30, False), (1e30, True)])
def test_emulation_within_the_stated_resolution_of_fp64(scale, hot):
    rng = np.random.default_rng(3)
    n, grid = 4000, (6, 7, 5)
    pts = rng.uniform(-0.14, 0.14, (n, 3)).astype(np.float32)
    if hot:
        pts[:3000] = np.float32([0.01, 0.02, -0.03])
    d_e = (rng.normal(size=(n, 32)) * scale).astype(np.float32)
    d_e[rng.random(n) < 0.3] = 0
    dense = 2 * n
    got = E.grid_backward_det(pts, d_e, grid, dense)
    ref = E.grid_backward_f64(pts, d_e, grid)
    # per voxel-channel: <= one rounding to the int64 grid per contribution, and the final rounding to fp32
    contrib = np.zeros((int(np.prod(grid)), 32))
    for ok, vox, _ in E.corners(pts, grid):
        r = np.nonzero(ok)[0]
        np.add.at(contrib, vox[r], (d_e[r] != 0).astype(np.float64))
    bound = contrib.reshape(ref.shape) * E.resolution(d_e, dense) + np.abs(ref) * 2.0 ** -24 + 1e-300
    err = np.abs(got.astype(np.float64) - ref)
    assert (err <= bound * 1.0001).all(), float((err / bound).max())
    assert np.abs(ref).max() > 0 and np.isfinite(got).all()
    # the resolution is far inside fp32: about 2^(e + h - 63) of the largest value
    assert E.resolution(d_e, dense) <= np.abs(d_e).max() * 2.0 ** -40


def test_emulation_is_order_independent_and_marks_nonfinite_values():
    rng = np.random.default_rng(4)
    n, grid = 3000, (5, 5, 5)
    pts = rng.uniform(-0.13, 0.13, (n, 3)).astype(np.float32)
    d_e = rng.normal(size=(n, 32)).astype(np.float32)
    d_e[17, 3] = np.nan
    d_e[99] = np.inf
    a = E.grid_backward_det(pts, d_e, grid, n)
    perm = rng.permutation(n)
    b = E.grid_backward_det(pts[perm], d_e[perm], grid, n)
    assert np.array_equal(a, b, equal_nan=True)
    bad = np.zeros((125, 32), dtype=bool)
    for ok, vox, _ in E.corners(pts, grid):
        for r, cs in ((17, [3]), (99, list(range(32)))):
            if ok[r]:
                bad[vox[r], cs] = True
    assert bad.any() and np.array_equal(np.isnan(a).reshape(-1, 32), bad)
    # the finite values alone set the scale: the NaN / Inf rows change nothing else
    clean = d_e.copy()
    clean[17, 3] = 0
    clean[99] = 0
    c = E.grid_backward_det(pts, clean, grid, n)
    assert np.array_equal(np.where(bad.reshape(a.shape), 0, a), np.where(bad.reshape(a.shape), 0, c))


def test_shift_uses_the_dense_row_count():
    d_e = np.float32([[0.75] + [0] * 31])       # 0.75 < 2^0
    assert E.shift(d_e, 1) == 62 and E.shift(d_e, 2) == 61 and E.shift(d_e, 1000) == 52 and E.shift(d_e, 1024) == 52
    assert E.shift(np.zeros((3, 32), np.float32), 3) == 60


def test_route_switch_follows_torch_unless_the_module_says():
    mod = S.TextureEmbeddingPiGAN128SEMANTICDISENTANGLE(hidden_dim=32, z_geo_dim=8, z_app_dim=8, output_dim=22)
    assert mod.deterministic_backward is None
    old = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled())
    try:
        torch.use_deterministic_algorithms(False)
        assert SA.deterministic_grid(mod) is False
        torch.use_deterministic_algorithms(True)
        assert SA.deterministic_grid(mod) is True
        mod.deterministic_backward = False
        assert SA.deterministic_grid(mod) is False
        torch.use_deterministic_algorithms(False)
        mod.deterministic_backward = True
        assert SA.deterministic_grid(mod) is True
    finally:
        torch.use_deterministic_algorithms(old[0], warn_only=old[1])


def test_new_entry_points_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "fenerf.h")).read()
    for name in ("fenerf_model_set_grid_grad_mode", "fenerf_grid_backward_det_workspace_bytes", "fenerf_grid_backward_det"):
        assert name + "(" in hdr and name in _lib.EXPORTS
    assert "#define FENERF_GRID_GRAD_ATOMIC 0" in hdr and "#define FENERF_GRID_GRAD_DETERMINISTIC 1" in hdr
    assert (_lib.GRID_GRAD_ATOMIC, _lib.GRID_GRAD_DETERMINISTIC) == (0, 1) and _lib.ABI_VERSION == 2
