"""Free camera, no device needed: the numpy emulation of fenerf_camera_rays against its fp64 definition, the reference's camera and the
CPU ray statement; windows; the Camera constructors; the torch statement's gradients against fp64 autograd; the tools' new flags."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import ray_tail_cases as RC
from conftest import ROOT
from fenerf_amd import camera_emulation as CE
from fenerf_amd.camera import Camera, rays_torch, rotation_exp
from fenerf_amd.generators import volumetric_rendering as VR

F = np.float32
EPS24 = 2.0 ** -24


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F)).view(np.uint32)


def _orthonormal(rng, B):
    q = np.linalg.qr(rng.normal(size=(B, 3, 3)))[0]
    return q * np.sign(np.linalg.det(q))[:, None, None]


def _random_case(rng, B=2):
    M = np.concatenate([_orthonormal(rng, B), rng.normal(size=(B, 3, 1))], -1).astype(F)
    fov = rng.uniform(5, 90, B)
    K = np.stack([rng.uniform(0.5, 2, B), rng.uniform(0.5, 2, B), rng.uniform(-0.5, 0.5, B), rng.uniform(-0.5, 0.5, B),
                  -1 / np.tan(np.radians(fov) / 2)], -1).astype(F)
    return M, K, (int(rng.integers(1, 41)), int(rng.integers(1, 41)))


def test_emulation_fp32_against_its_fp64_definition():
    """200 random cameras: every dirs component of the fp32 statement within 8 * 2^-24 of the same statement in fp64 (the count of roundings
    on unit-scale values: grid 2, offset and scale 2, norm 3, quotient 1, the 3-term product sum 3 -- each at most half an ulp of a value
    <= 1 in a unit vector's chain); origins are column 3's bits; the depths are VR.sample_rays(..., 'cpu')'s bits for the same jitter."""
    rng = np.random.default_rng(2024)
    worst, squares = 0.0, 0
    for case in range(200):
        M, K, (W, H) = _random_case(rng)
        if case % 4 == 0:
            H = W                      # every fourth case square: the CPU ray statement the depths are compared with takes square images
        N = int(rng.integers(1, 14))
        u = rng.random((2, W * H, N, 1)).astype(F)
        rs, re = (0.88, 1.12) if case % 2 else (0.1, 5.0)
        o32, d32, z32 = CE.camera_rays(M, K, (W, H), None, N, rs, re, u, np.float32)
        o64, d64, _ = CE.camera_rays(M, K, (W, H), None, N, rs, re, u, np.float64)
        assert d32.dtype == F and d64.dtype == np.float64 and d32.shape == (2, W * H, 3)
        worst = max(worst, float(np.abs(d32 - d64).max()))
        assert np.array_equal(_bits(o32), _bits(np.broadcast_to(M[:, None, :, 3], o32.shape)))
        if W == H:
            z_cpu = VR.sample_rays(2, N, "cpu", 12, (W, H), rs, re, 0.0, 0.0, 0.3, 1.0, "mean", draws=VR.RecordedDraws([u]))[2]
            assert np.array_equal(_bits(z32), _bits(z_cpu.numpy())), (case, W, N)
            squares += 1
    assert squares >= 50
    print(f"[camera] emulation fp32 vs fp64 over 200 cases: worst |dirs error| {worst / EPS24:.2f} * 2^-24")
    assert worst <= 8 * EPS24


@pytest.mark.parametrize("S,N,fov,ray_range", RC.RAY_SETUP_CASES)
def test_the_references_camera(S, N, fov, ray_range):
    """intrinsics (1, 1, 0, 0, zc) and the look-at matrix rebuilt in fp32 by ray_setup_kernel's steps: the oracle's ray setup within the
    bound tests/test_gpu_ray_tail.py holds the kernel to"""
    u = RC.ray_setup_jitter(S, N)
    pitch = RC.clamped_pitch(RC.RAY_PHI)
    sp, cp, st, ct = np.sin(pitch), np.cos(pitch), np.sin(RC.RAY_THETA), np.cos(RC.RAY_THETA)
    origin = np.stack([sp * ct, cp, sp * st], -1).astype(F)
    got = CE.camera_rays(CE.lookat_cam2world(origin), CE.reference_intrinsics(fov, 3), (S, S), None, N, ray_range[0], ray_range[1], u)
    r64 = RC.oracle_ray_setup(S, N, fov, ray_range, u, RC.RAY_THETA, pitch, np.float64)
    r32 = RC.oracle_ray_setup(S, N, fov, ray_range, u, RC.RAY_THETA, pitch, np.float32)
    for name, g, a, b in zip(("origins", "dirs", "z"), got, r64, r32):
        err, e32 = RC.max_err(g, a), RC.max_err(b, a)
        bound = 4 * e32 + 8 * EPS24 * max(1.0, float(np.abs(a).max()))
        assert g.dtype == F and np.isfinite(g).all() and err <= bound, (name, err, bound)


WINDOWS = {(5, 3): [(0, 0, 5, 3), (0, 0, 2, 2), (3, 1, 2, 2), (4, 2, 1, 1), (0, 2, 5, 1), (1, 1, 3, 1)],
           (17, 9): [(0, 0, 17, 1), (16, 0, 1, 9), (0, 8, 17, 1), (0, 0, 1, 9), (5, 3, 7, 4), (8, 4, 1, 1)],
           (16, 16): [(0, 0, 8, 8), (8, 0, 8, 8), (0, 8, 8, 8), (8, 8, 8, 8), (15, 0, 1, 16), (7, 7, 1, 1)]}


@pytest.mark.parametrize("size", sorted(WINDOWS))
def test_windows_are_the_full_grids_rays(size):
    rng = np.random.default_rng(size[0])
    M, K, _ = _random_case(rng)
    W, H = size
    N = 3
    u = rng.random((2, H, W, N)).astype(F)
    o, d, z = (a.reshape(2, H, W, -1) for a in CE.camera_rays(M, K, size, None, N, 0.88, 1.12, u))
    cam = Camera(torch.from_numpy(M), torch.from_numpy(K), size)
    o_t, d_t = (a.reshape(2, H, W, 3).numpy() for a in rays_torch(cam.cam2world, cam.intrinsics, size))
    for x0, y0, w, h in WINDOWS[size]:
        cut = lambda a: np.ascontiguousarray(a[:, y0:y0 + h, x0:x0 + w]).reshape(2, w * h, -1)
        got = CE.camera_rays(M, K, size, (x0, y0, w, h), N, 0.88, 1.12, cut(u))
        for name, g, full in zip(("origins", "dirs", "z"), got, (o, d, z)):
            assert np.array_equal(_bits(g), _bits(cut(full))), (name, x0, y0, w, h)
        # the torch statement and Camera.crop: the same property (a window of a window included)
        c = cam.crop(x0, y0, w, h)
        assert c.window == (x0, y0, w, h) and c.frame == (w, h)
        ow, dw, zw = c.rays(N, 0.88, 1.12, VR.RecordedDraws([cut(u)[..., None]]))
        assert np.array_equal(_bits(dw.numpy()), _bits(cut(d_t))) and np.array_equal(_bits(ow.numpy()), _bits(cut(o_t)))
        assert np.array_equal(_bits(zw.numpy()), _bits(cut(z)))
        if w > 1:
            assert c.crop(1, 0, w - 1, h).window == (x0 + 1, y0, w - 1, h)
    for bad in ((-1, 0, 1, 1), (0, 0, W + 1, 1), (0, H, 1, 1), (0, 0, 0, 1)):
        with pytest.raises(ValueError):
            cam.crop(*bad)
        with pytest.raises(ValueError):
            CE.window_grid(size, bad)


def test_camera_constructors():
    theta = torch.tensor(RC.RAY_THETA).reshape(-1, 1)
    phi = torch.tensor(RC.RAY_PHI).reshape(-1, 1)
    cam = Camera.from_angles(theta, phi, 12, (8, 8))
    origin, _, _ = VR.camera_position(theta, phi)
    rot = VR._lookat_rotation(VR.normalize_vecs(-origin))
    assert cam.cam2world.shape == (3, 3, 4) and cam.batch == 3 and cam.frame == (8, 8)
    assert np.array_equal(_bits(cam.cam2world[:, :, :3].numpy()), _bits(rot.numpy()))
    assert np.array_equal(_bits(cam.cam2world[:, :, 3].numpy()), _bits(origin.numpy()))
    z_cam = (-torch.ones(1) / np.tan((2 * math.pi * 12 / 360) / 2)).item()
    assert np.array_equal(_bits(cam.intrinsics.numpy()), _bits(np.tile(np.array([1, 1, 0, 0, z_cam], dtype=F), (3, 1))))
    assert np.array_equal(_bits(CE.reference_intrinsics(12, 3)), _bits(cam.intrinsics.numpy()))
    # radius: the position scales, the axes stay
    far = Camera.from_angles(theta, phi, 12, (8, 8), radius=2.5)
    np.testing.assert_allclose(far.cam2world[:, :, 3].numpy(), 2.5 * origin.numpy(), rtol=1e-6)
    np.testing.assert_allclose(far.cam2world[:, :, :3].numpy(), rot.numpy(), atol=1e-6)
    # roll: right / up rotate about the view axis, which stays
    a = 0.4
    rolled = Camera.from_angles(theta, phi, 12, (8, 8), roll=a).cam2world
    right, up = rot[:, :, 0], rot[:, :, 1]
    np.testing.assert_allclose(rolled[:, :, 0].numpy(), (math.cos(a) * right + math.sin(a) * up).numpy(), atol=1e-6)
    np.testing.assert_allclose(rolled[:, :, 1].numpy(), (math.cos(a) * up - math.sin(a) * right).numpy(), atol=1e-6)
    assert torch.equal(rolled[:, :, 2:], cam.cam2world[:, :, 2:])
    # look_at from the same positions: the same camera
    la = Camera.look_at(origin, torch.zeros(3), (0.0, 1.0, 0.0), 12, (8, 8))
    np.testing.assert_allclose(la.cam2world.numpy(), cam.cam2world.numpy(), atol=2e-6)
    # perturbed(0, 0): the identity -- every value equal (R @ I turns a -0 entry into +0: equal, not the same bits)
    zero = torch.zeros(3, 3)
    same = cam.perturbed(zero, zero, torch.zeros(3))
    assert torch.equal(same.cam2world, cam.cam2world) and same.window == cam.window
    assert np.array_equal(_bits(same.intrinsics.numpy()), _bits(cam.intrinsics.numpy())) and same.size == cam.size
    # d exp / d rotvec at 0: the three generators, finite
    jac = torch.autograd.functional.jacobian(lambda r: rotation_exp(r.reshape(1, 3))[0], torch.zeros(3, dtype=torch.float64))   # [3,3,3]
    for k in range(3):
        e = np.zeros(3)
        e[k] = 1
        gen = np.array([[0, -e[2], e[1]], [e[2], 0, -e[0]], [-e[1], e[0], 0]])
        assert np.isfinite(jac[..., k].numpy()).all() and np.abs(jac[..., k].numpy() - gen).max() <= 1e-6
    # the series and the closed form meet; a finite rotation is a rotation
    r = torch.tensor([[0.3, -0.2, 0.9], [0.006, 0.004, -0.002], [0.0099, 0.0, 0.0]], dtype=torch.float64)
    Rm = rotation_exp(r)
    np.testing.assert_allclose((Rm @ Rm.transpose(1, 2)).numpy(), np.tile(np.eye(3), (3, 1, 1)), atol=1e-12)
    c, s = math.cos(0.0099), math.sin(0.0099)
    np.testing.assert_allclose(Rm[2].numpy(), np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), atol=1e-14)
    with pytest.raises(ValueError):
        Camera(torch.zeros(2, 3, 4), torch.zeros(3, 5), (4, 4))
    with pytest.raises(ValueError):
        Camera(torch.zeros(1, 3, 4), torch.zeros(1, 5), (4, 4), window=(2, 2, 3, 1))


def test_torch_statement_gradients_against_fp64_autograd():
    """Camera.rays on the CPU (fp32 torch statement) -> cam2world.grad / intrinsics.grad against fp64 autograd of the emulation's formula
    (camera_grad_terms: the analytic per-ray terms, summed in fp64 -- themselves checked against fp64 autograd here), 1e-5 relative max-norm"""
    rng = np.random.default_rng(5)
    for size, window in (((9, 7), None), ((16, 16), (3, 2, 6, 11)), ((1, 1), None)):
        M, K, _ = _random_case(rng, B=2)
        cam = Camera(torch.from_numpy(M).requires_grad_(), torch.from_numpy(K).requires_grad_(), size, window)
        w, h = cam.frame
        g_o, g_d = rng.normal(size=(2, w * h, 3)), rng.normal(size=(2, w * h, 3))
        o, d, z = cam.rays(4, 0.88, 1.12)
        assert not z.requires_grad and z.shape == (2, w * h, 4)
        ((o * torch.from_numpy(g_o).float()).sum() + (d * torch.from_numpy(g_d).float()).sum()).backward()
        # fp64 autograd of the formula
        M64, K64 = torch.from_numpy(M).double().requires_grad_(), torch.from_numpy(K).double().requires_grad_()
        o64, d64 = rays_torch(M64, K64, size, window)
        ((o64 * torch.from_numpy(g_o)).sum() + (d64 * torch.from_numpy(g_d)).sum()).backward()
        ref = np.concatenate([M64.grad.numpy().reshape(2, 12), K64.grad.numpy()], -1)
        terms = CE.camera_grad_terms(M, K, size, window, g_o, g_d).sum(1)
        assert np.abs(terms - ref).max() <= 1e-9 * np.abs(ref).max(), "camera_grad_terms is the gradient of the emulation's formula"
        got = np.concatenate([cam.cam2world.grad.numpy().reshape(2, 12), cam.intrinsics.grad.numpy()], -1)
        for name, sl in (("cam2world", slice(0, 12)), ("intrinsics", slice(12, 17))):
            rel = np.abs(got[:, sl] - ref[:, sl]).max() / np.abs(ref[:, sl]).max()
            assert rel <= 1e-5, (name, size, window, rel)
    # a NULL input's terms are zero
    t = CE.camera_grad_terms(M, K, size, window, None, g_d)
    assert not t[..., [3, 7, 11]].any() and t[..., :3].any()
    t = CE.camera_grad_terms(M, K, size, window, g_o, None)
    assert not t[..., [0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13, 14, 15, 16]].any() and t[..., 3].any()


def _refused(parse, argv, capsys):
    with pytest.raises(SystemExit) as e:
        parse(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


def test_cli_flags(capsys):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import inverse_render
        import render_multiview
    finally:
        sys.path.pop(0)
    o = render_multiview.parse_options(["g.pth", "--roll", "15", "--radius", "1.3", "--crop", "8", "16", "32", "24", "--image_size", "64"])
    assert o.roll == 15.0 and o.radius == 1.3 and o.crop == [8, 16, 32, 24] and render_multiview.uses_camera(o)
    o = render_multiview.parse_options(["g.pth"])
    assert o.roll is None and o.radius is None and o.crop is None and not render_multiview.uses_camera(o)
    assert "outside" in _refused(render_multiview.parse_options, ["g.pth", "--image_size", "64", "--crop", "40", "0", "32", "8"], capsys)
    assert "outside" in _refused(render_multiview.parse_options, ["g.pth", "--image_size", "64", "--crop", "0", "60", "8", "8"], capsys)
    _refused(render_multiview.parse_options, ["g.pth", "--crop", "0", "0", "8", "8", "--labels_only"], capsys)
    o = inverse_render.parse_options(["n", "g.pth", "--optimize_pose", "--pose_model", "se3", "--optimize_focal"])
    assert o.pose_model == "se3" and o.optimize_focal is True
    o = inverse_render.parse_options(["n", "g.pth", "--optimize_pose"])
    assert o.pose_model == "angles" and o.optimize_focal is False
    assert "se3" in _refused(inverse_render.parse_options, ["n", "g.pth", "--optimize_pose", "--optimize_focal"], capsys)
    assert "optimize_pose" in _refused(inverse_render.parse_options, ["n", "g.pth", "--pose_model", "se3"], capsys)
    # the library calls refuse the same combinations
    from fenerf_amd import callers
    for kw in (dict(pose_model="se3"), dict(optimize_pose=True, optimize_focal=True), dict(optimize_pose=True, pose_model="quaternion")):
        with pytest.raises(ValueError):
            callers.inverse_render(None, None, None, {}, **kw)
    with pytest.raises(ValueError):
        callers.render_multiview(None, {0: {"num_steps": 1}}, 0, "cpu", cameras=[None], labels_only=True)
    with pytest.raises(ValueError, match="empty"):
        callers.render_multiview(None, {0: {"num_steps": 1}}, 0, "cpu", cameras=[])


def test_library_declares_the_camera_entries():
    from fenerf_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "fenerf.h")).read()
    l = _lib.lib()
    for name, n_args in (("fenerf_camera_rays", 17), ("fenerf_camera_grads", 16), ("fenerf_camera_grads_workspace_bytes", 2),
                         ("fenerf_camera_grads_chain_length", 1)):
        assert name + "(" in hdr and name in _lib.EXPORTS and hasattr(l, name) and len(_lib._SIGS[name][1]) == n_args
    # the chain length the header promises: at most 64 additions for every R up to 2^20, and growing with neither B nor small R
    L = [l.fenerf_camera_grads_chain_length(R) for R in (1, 64, 257, 4097, 1 << 14, 1 << 18, (1 << 20) - 1, 1 << 20)]
    assert all(0 < v <= 64 for v in L) and l.fenerf_camera_grads_chain_length(0) == 0
    assert l.fenerf_camera_grads_workspace_bytes(3, 4097) == 3 * l.fenerf_camera_grads_workspace_bytes(1, 4097) > 0
