"""Camera-pose gradients, the parts that need no device: the torch formulation of the rays (volumetric_rendering.rays_from_angles, the
graph a pose that requires grad reaches the rays through) and the argument checks of fenerf_ray_grads / fenerf_render_backward_rays."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from fenerf_amd import _lib
from fenerf_amd.generators import volumetric_rendering as VR


def _rays64(yaw, pitch):
    origins, dirs, _, _ = VR.rays_from_angles(yaw.reshape(1, 1), pitch.reshape(1, 1), (3, 3), 12, "cpu")
    return origins, dirs


@pytest.mark.parametrize("yaw,pitch", [(math.pi / 2, math.pi / 2), (math.pi / 2 + 0.3, math.pi / 2 - 0.155), (0.4, 2.6)])
def test_rays_from_angles_gradcheck(yaw, pitch):
    """fp64 gradcheck of origins / dirs of a 3 x 3 camera wrt yaw and pitch, away from the pitch clamp"""
    y = torch.tensor(yaw, dtype=torch.float64, requires_grad=True)
    p = torch.tensor(pitch, dtype=torch.float64, requires_grad=True)
    o, d = _rays64(y, p)
    assert o.dtype == torch.float64 and d.dtype == torch.float64 and o.shape == (1, 9, 3) and d.shape == (1, 9, 3)
    assert torch.autograd.gradcheck(_rays64, (y, p), eps=1e-6, atol=1e-8, rtol=1e-6)


@pytest.mark.parametrize("pitch", [0.0, -0.3, math.pi, 4.0])
def test_pitch_at_the_clamp_has_zero_gradient(pitch):
    """sample_camera_positions clamps phi to [1e-5, pi - 1e-5] (volumetric_rendering.py:220): where the clamp binds the rays do not depend
    on the pitch -- a zero gradient, not a NaN -- and the yaw gradient is still there"""
    y = torch.tensor(1.1, dtype=torch.float64, requires_grad=True)
    p = torch.tensor(pitch, dtype=torch.float64, requires_grad=True)
    o, d = _rays64(y, p)
    w = torch.linspace(-1, 1, 27, dtype=torch.float64).reshape(1, 9, 3)
    ((o * w).sum() + (d * w.flip(1)).sum()).backward()
    assert p.grad is not None and float(p.grad) == 0.0
    assert torch.isfinite(y.grad) and float(y.grad.abs()) > 0


@pytest.mark.parametrize("mode,h_std,v_std", [(None, 0, 0), ("gaussian", 0.3, 0.155), ("uniform", 0.2, 0.1)])
def test_rays_from_angles_is_sample_rays_cpu_branch_bit_for_bit(mode, h_std, v_std):
    """sample_rays' non-GPU branch is the factored function on the angles it draws: same values bit for bit, same draws in the same order
    (jitter, theta, phi), and equal to the reference-shaped transform_sampled_points within fp32 rounding"""
    n, N, res, fov = 2, 5, (4, 4), 12
    torch.manual_seed(5)
    origins, dirs, z, pitch, yaw = VR.sample_rays(n, N, "cpu", fov, res, 0.88, 1.12, h_std, v_std, 1.3, 1.7, mode)
    after = torch.rand(1)
    torch.manual_seed(5)
    VR._DEFAULT_DRAWS.rand((n, 16, N, 1), "cpu")
    theta, phi = VR.sample_camera_angles("cpu", n, h_std, v_std, 1.3, 1.7, mode)
    o2, d2, pitch2, yaw2 = VR.rays_from_angles(theta, phi, res, fov, "cpu")
    assert torch.equal(after, torch.rand(1)), "same number of draws"
    for a, b in ((origins, o2), (dirs, d2), (pitch, pitch2), (yaw, yaw2)):
        assert a.dtype == torch.float32 and torch.equal(a, b)
    torch.manual_seed(5)
    pts, zv, d_cam = VR.get_initial_rays_trig(n, N, "cpu", fov, res, 0.88, 1.12)
    _, z3, d3, o3, pitch3, yaw3 = VR.transform_sampled_points(pts, zv, d_cam, "cpu", h_std, v_std, 1.3, 1.7, mode)
    assert torch.equal(pitch3, pitch) and torch.equal(yaw3, yaw) and torch.equal(o3, origins)
    assert float((d3 - dirs).abs().max()) <= 1e-6 and float((z3.squeeze(-1) - z).abs().max()) <= 1e-6


def test_pose_tensors_reach_the_rays_on_the_cpu_branch():
    """h_mean / v_mean as 0-dim tensors that require grad: the CPU branch's rays and the returned pitch / yaw carry their graph"""
    y = torch.tensor(1.4, requires_grad=True)
    p = torch.tensor(1.6, requires_grad=True)
    torch.manual_seed(1)
    origins, dirs, z, pitch, yaw = VR.sample_rays(1, 4, "cpu", 12, (3, 3), 0.88, 1.12, 0.3, 0.155, y, p, "gaussian")
    assert origins.requires_grad and dirs.requires_grad and pitch.requires_grad and yaw.requires_grad and not z.requires_grad
    (origins.sum() + dirs[..., 0].sum() + pitch.sum() + 2 * yaw.sum()).backward()
    assert float(y.grad.abs()) > 0 and float(p.grad.abs()) > 0


def test_ray_grads_argument_checks_need_no_device():
    """fenerf_ray_grads / fenerf_render_backward_rays refuse bad arguments before they touch the device"""
    l = _lib.lib()
    assert "fenerf_ray_grads" in _lib.EXPORTS and "fenerf_render_backward_rays" in _lib.EXPORTS and \
        "fenerf_render_backward_rays_workspace_bytes" in _lib.EXPORTS
    buf = (C.c_float * 4096)()
    p = C.cast(buf, C.c_void_p)
    bad = [
        ((0, 2, 4, 1, p, None, p, None, p, p, None), "B, R > 0"),
        ((1, 0, 4, 1, p, None, p, None, p, p, None), "B, R > 0"),
        ((1, 2, 2, 1, p, None, p, None, p, p, None), "num_steps"),
        ((1, 2, 513, 1, p, None, p, None, p, p, None), "num_steps"),
        ((1, 2, 4, 3, p, None, p, None, p, p, None), "passes"),
        ((1, 2, 4, 0, p, None, p, None, p, p, None), "passes"),
        ((1, 2, 4, 1, None, None, p, None, p, p, None), "d_points"),
        ((1, 2, 4, 1, p, None, None, None, p, p, None), "z_coarse"),
        ((1, 2, 4, 2, p, None, p, None, p, p, None), "z_fine"),
        ((1, 2, 4, 1, p, None, p, p, p, p, None), "z_fine"),
        ((1, 2, 4, 1, p, None, p, None, None, None, None), "both NULL"),
    ]
    for args, word in bad:
        rc = l.fenerf_ray_grads(*args)
        assert rc == _lib.E_INVALID, (args, rc)
        assert word in l.fenerf_last_error().decode(), (word, l.fenerf_last_error().decode())
    opts = _lib.composite_opts("relu")
    g = _lib.FenerfSirenGrads()
    rc = l.fenerf_render_backward_rays(None, 1, 4, 4, 0, p, 16, 0, p, None, C.byref(opts), p, C.byref(g), None, None, 0, 0, p, 16, p, p, 3, p, p, None)
    assert rc == _lib.E_INVALID and "model is NULL" in l.fenerf_last_error().decode()
    assert l.fenerf_render_backward_rays_workspace_bytes(None, 1, 4, 4, 0, 0, 0, 0) == 0
