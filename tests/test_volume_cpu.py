"""The baked radiance lattice as include/fenerf.h states it, on its numpy restatement (fenerf_amd/volume_emulation.py -- the yardstick
the GPU tests hold fenerf_volume_sample to), the host arithmetic of callers.baked_cube_length, and the declarations.  Nothing here touches
the kernels."""
import functools
import math
import os

import numpy as np
import torch

from conftest import ROOT
from fenerf_amd import volume_emulation as V

SHAPE, C = (5, 4, 3), 3
ORIGIN, SPACING = (-4.0, 1.0, -0.5), (0.5, 0.25, 2.0)        # powers of two: the lattice nodes are hit exactly
OUT = -7.0


@functools.lru_cache(maxsize=None)
def lattice():
    vol = np.random.default_rng(0).uniform(-1, 1, SHAPE + (C,)).astype(np.float32)
    vol.setflags(write=False)
    return vol


def node_points(shape=SHAPE, origin=ORIGIN, spacing=SPACING):
    idx = np.stack(np.meshgrid(*(np.arange(n) for n in shape), indexing="ij"), -1).reshape(-1, 3)
    return idx, (np.asarray(origin, np.float32) + idx.astype(np.float32) * np.asarray(spacing, np.float32)).astype(np.float32)


def test_emulation_against_fp64_grid_sample():
    """2,000 random inside points against F.grid_sample(bilinear, align_corners=True) in fp64.  Bound (derived, not measured): three lerp
    levels of at most three roundings each, plus the two roundings of t scaled by the index range: (16 + 4 max n_k) 2^-24 max|vol|."""
    vol = lattice()
    rng = np.random.default_rng(1)
    t = rng.uniform(0, 1, (2000, 3)) * (np.array(SHAPE) - 1)
    pts = (np.array(ORIGIN) + t * np.array(SPACING)).astype(np.float32)
    got = V.sample(vol, ORIGIN, SPACING, pts, OUT)
    assert got.dtype == np.float32 and got.shape == (2000, C)
    # grid_sample: input [1, C, D, H, W] = axes (0, 1, 2); grid[..., (x, y, z)] addresses (W, H, D) = axes (2, 1, 0), in [-1, 1]
    t64 = (pts.astype(np.float64) - np.array(ORIGIN)) / np.array(SPACING)
    g = 2.0 * t64 / (np.array(SHAPE) - 1) - 1.0
    grid = torch.from_numpy(g[:, ::-1].copy()).reshape(1, 1, 1, -1, 3)
    inp = torch.from_numpy(vol.astype(np.float64)).permute(3, 0, 1, 2)[None]
    ref = torch.nn.functional.grid_sample(inp, grid, mode="bilinear", align_corners=True)[0, :, 0, 0].t().numpy()
    bound = (16 + 4 * max(SHAPE)) * 2.0 ** -24 * float(np.abs(vol).max())
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"emulation vs fp64 grid_sample: max |err| {err:.3e}, bound {bound:.3e}")
    assert err <= bound


def test_nodes_and_planes_bit_for_bit():
    vol = lattice()
    idx, pts = node_points()
    got = V.sample(vol, ORIGIN, SPACING, pts, OUT)
    want = vol[idx[:, 0], idx[:, 1], idx[:, 2]]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))          # the planes t = 0 and t = n - 1 included


def test_outside_points_and_nan_lattice_value():
    vol = lattice()
    o, s = np.array(ORIGIN, np.float32), np.array(SPACING, np.float32)
    mid = (o + s * np.float32(0.5)).astype(np.float32)
    bad = []
    for k in range(3):
        above = np.float32(o[k] + (SHAPE[k] - 1) * s[k])          # the first coordinate whose t, as fp32 rounds it, exceeds n - 1
        for _ in range(16):
            if np.float32(np.float32(above - o[k]) / s[k]) > np.float32(SHAPE[k] - 1):
                break
            above = np.nextafter(above, np.float32(np.inf))
        assert np.float32(np.float32(above - o[k]) / s[k]) > np.float32(SHAPE[k] - 1)
        for v in (np.nextafter(o[k], np.float32(-np.inf)), above, np.nan, np.inf, -np.inf):
            p = mid.copy()
            p[k] = v
            bad.append(p)
    got = V.sample(vol, ORIGIN, SPACING, np.array(bad, np.float32), OUT)
    want = np.zeros((len(bad), C), np.float32)
    want[:, -1] = OUT
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # a NaN lattice value reaches the rows of its eight neighbouring cells and nothing else
    poisoned = vol.copy()
    node = (2, 1, 1)
    poisoned[node + (1,)] = np.nan
    rng = np.random.default_rng(2)
    t = rng.uniform(0, 1, (3000, 3)) * (np.array(SHAPE) - 1)
    pts = (np.array(ORIGIN) + t * np.array(SPACING)).astype(np.float32)
    clean, dirty = V.sample(vol, ORIGIN, SPACING, pts, OUT), V.sample(poisoned, ORIGIN, SPACING, pts, OUT)
    tt = (pts - o) / s
    cell = np.minimum(np.floor(tt).astype(int), np.array(SHAPE) - 2)
    touches = np.all((cell <= np.array(node)) & (np.array(node) <= cell + 1), axis=1)
    assert touches.any() and (~touches).any()
    assert np.isnan(dirty[touches, 1]).all()                                  # 0 * NaN included: a point on the cell's far face too
    assert np.array_equal(dirty[~touches].view(np.uint32), clean[~touches].view(np.uint32))
    assert np.array_equal(np.delete(dirty, 1, axis=1).view(np.uint32), np.delete(clean, 1, axis=1).view(np.uint32))   # other channels untouched


def test_baked_cube_length_holds_every_sample_and_is_tight():
    """200 random poses (yaw uniform over the circle, pitch uniform over (0, pi)) of the package's own sample_rays on the CPU at img_size 8,
    N = 6 with the curriculum's camera: every (jittered) sample lies inside the cube, and a cube 2 % smaller loses a sample."""
    from fenerf_amd import callers, curriculums
    from fenerf_amd.generators.volumetric_rendering import sample_rays
    cur = curriculums.CelebA_double_semantic
    fov, rs, re = cur["fov"], cur["ray_start"], cur["ray_end"]
    N, S, n_poses = 6, 8, 200
    side = callers.baked_cube_length(fov, rs, re, num_steps=N)
    # the formula, restated: camera on the unit sphere, corner ray at tan(theta_c) = sqrt(2) tan(fov / 2), depths half a bin beyond either end
    h = (re - rs) / (N - 1) / 2
    cc = math.cos(math.atan(math.sqrt(2) * math.tan(math.radians(fov) / 2)))
    assert math.isclose(side, 2 * max(math.sqrt(1 + z * z - 2 * z * cc) for z in (rs - h, re + h)), rel_tol=1e-12)
    assert callers.baked_cube_length(fov, rs, re) < side                       # without the jitter margin: the plain ends
    assert math.isclose(callers.baked_cube_length(fov, rs, re, radius=2.0, num_steps=N),
                        2 * max(math.sqrt(4 + z * z - 4 * z * cc) for z in (rs - h, re + h)), rel_tol=1e-12)
    torch.manual_seed(0)
    yaw = torch.rand(n_poses, 1) * 2 * math.pi
    pitch = torch.rand(n_poses, 1) * math.pi
    reach = _reach(sample_rays(n_poses, N, "cpu", fov, (S, S), rs, re, 0, 0, yaw, pitch, None))
    print(f"baked_cube_length {side:.6f}: largest |coordinate| over {n_poses} random poses {reach:.6f} = {2 * reach / side:.4f} of the half side; "
          f"without the jitter margin the half side would be {callers.baked_cube_length(fov, rs, re) / 2:.6f}")
    assert reach <= side / 2
    # tight, not merely generous: the pose (on a 2-degree grid) whose far corner sample lies closest to a coordinate axis, drawn 200 times --
    # the jitter of that sample is then within a tenth of a bin of its end in some draw (all but 0.9^200 of the time), which is 98.4 % of the half side
    from fenerf_amd.generators.volumetric_rendering import rays_from_angles
    gy, gp = torch.meshgrid(torch.arange(0.0, 360.0, 2.0), torch.arange(2.0, 180.0, 2.0), indexing="ij")
    gy, gp = torch.deg2rad(gy).reshape(-1, 1), torch.deg2rad(gp).reshape(-1, 1)
    o, d, _, _ = rays_from_angles(gy, gp, (S, S), fov, "cpu")
    far = (o + d * (re + h)).abs().amax(dim=(1, 2))
    worst = int(far.argmax())
    reach_w = _reach(sample_rays(n_poses, N, "cpu", fov, (S, S), rs, re, 0, 0, gy[worst].expand(n_poses, 1), gp[worst].expand(n_poses, 1), None))
    print(f"worst grid pose yaw {float(gy[worst]):.4f} pitch {float(gp[worst]):.4f}: largest |coordinate| {reach_w:.6f} = {2 * reach_w / side:.4f} of the half side")
    assert reach_w <= side / 2
    assert reach_w > 0.98 * side / 2           # a cube 2 % smaller loses this sample


def _reach(rays):
    o, d, z = rays[:3]
    return float((o.unsqueeze(2) + d.unsqueeze(2) * z.unsqueeze(-1)).abs().max())


def test_volume_entry_points_are_declared_exported_and_reachable():
    import sys
    from fenerf_amd import _lib, callers, native
    hdr = open(os.path.join(ROOT, "include", "fenerf.h")).read()
    names = ("fenerf_volume_sample", "fenerf_volume_sample_rays", "fenerf_volume_render_workspace_bytes", "fenerf_volume_render")
    l = _lib.lib()
    for name in names:
        assert name + "(" in hdr and name in _lib.EXPORTS and hasattr(l, name)
    assert "#define FENERF_ABI_VERSION 2" in hdr and "#define FENERF_N_PHASES 17" in hdr
    for f in (native.volume_sample, native.volume_sample_rays, native.volume_render, callers.bake_field, callers.baked_cube_length):
        assert callable(f)
    assert callable(callers.BakedField.sample) and callable(callers.BakedField.render)
    # sizes need no device; invalid arguments give 0
    pts = 2 * 16 * 12
    assert l.fenerf_volume_render_workspace_bytes(2, 16, 12, 22, 0) == pts * 22 * 4
    hier = l.fenerf_volume_render_workspace_bytes(2, 16, 12, 22, 1)
    assert 2 * pts * 22 * 4 + 2 * pts * 4 <= hier <= 2 * pts * 22 * 4 + 2 * pts * 4 + 4 * 256
    assert l.fenerf_volume_render_workspace_bytes(2, 16, 12, 1, 1) == 0 and l.fenerf_volume_render_workspace_bytes(0, 16, 12, 22, 1) == 0
    # the tools pass --baked through; the defaults are the exact renders
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import inverse_render
        import render_multiview
    finally:
        sys.path.pop(0)
    assert render_multiview.build_parser().parse_args(["g.pth"]).baked is None
    assert render_multiview.build_parser().parse_args(["g.pth", "--baked", "128"]).baked == 128
    assert inverse_render.build_parser().parse_args(["n", "g.pth"]).baked is None
    assert inverse_render.build_parser().parse_args(["n", "g.pth", "--recon", "--baked", "256"]).baked == 256
