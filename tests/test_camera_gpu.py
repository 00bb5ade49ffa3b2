"""Free camera on the device: fenerf_camera_rays against its numpy emulation and against fenerf_ray_setup, fenerf_camera_grads against
the fp64 per-ray terms, the C-ABI's refusals, and the generator / callers entries that take a Camera."""
import ctypes as C
import functools
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

import ray_tail_cases as RC
from conftest import GOLDEN, ROOT
from test_gpu_parity import DEV, N_, T, _siren_module, load_golden
from test_gpu_pose_grads import _FixedDraws, _double_generator
from fenerf_amd import _lib, callers, camera_emulation as CE, native
from fenerf_amd.camera import Camera
from fenerf_amd.generators import generators as G
from fenerf_amd.siren import siren as S
from fenerf_amd.generators import volumetric_rendering as VR

pytestmark = pytest.mark.gpu
F = np.float32
EPS24 = 2.0 ** -24


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F)).view(np.uint32)


def _same_bits(name, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == F, (name, got.shape, want.shape, got.dtype)
    bad = _bits(got) != _bits(want)
    both_nan = np.isnan(got) & np.isnan(want)           # NaNs equal, whatever their payload
    assert not (bad & ~both_nan).any(), f"{name}: {int((bad & ~both_nan).sum())} of {got.size} values differ"


def _camera(rng, B, plain):
    """plain: orthonormal axes, centred unit intrinsics; else a sheared, scaled matrix and off-centre, anisotropic intrinsics"""
    q = np.linalg.qr(rng.normal(size=(B, 3, 3)))[0]
    if not plain:
        q = q @ (np.eye(3) + 0.3 * rng.normal(size=(B, 3, 3)))
    M = np.concatenate([q, rng.normal(size=(B, 3, 1))], -1).astype(F)
    fov = rng.uniform(5, 90, B)
    zc = -1 / np.tan(np.radians(fov) / 2)
    one, zero = np.ones(B), np.zeros(B)
    K = np.stack([one, one, zero, zero, zc] if plain else
                 [rng.uniform(0.5, 2, B), rng.uniform(0.5, 2, B), rng.uniform(-0.5, 0.5, B), rng.uniform(-0.5, 0.5, B), zc], -1).astype(F)
    return M, K


# ---------------------------------------------------------------------------------------------------
# 7. forward kernel against the emulation
# ---------------------------------------------------------------------------------------------------
GRIDS = [(1, 1, None), (5, 3, (1, 1, 3, 2)), (17, 9, None), (16, 16, (15, 0, 1, 16)), (64, 4, None)]


@pytest.mark.parametrize("N", [1, 2, 13])
@pytest.mark.parametrize("W,H,window", GRIDS)
@pytest.mark.parametrize("B", [1, 3])
def test_camera_rays_kernel_is_the_emulation(B, W, H, window, N):
    case = GRIDS.index((W, H, window)) + 5 * [1, 2, 13].index(N) + 15 * (B == 3)
    rng = np.random.default_rng(100 + case)
    M, K = _camera(rng, B, plain=case % 2 == 0)
    w, h = (W, H) if window is None else window[2:]
    u = rng.random((B, w * h, N)).astype(F)
    rs, re = (0.88, 1.12) if case % 3 else (0.1, 5.0)
    got = native.camera_rays(T(M), T(K), (W, H), window, N, rs, re, T(u))
    want = CE.camera_rays(M, K, (W, H), window, N, rs, re, u)
    for name, g, r in zip(("origins", "dirs", "z"), got, want):
        _same_bits(f"{name} B={B} {W}x{H} {window} N={N}", N_(g), r)


def test_camera_rays_nan_stays_in_its_image():
    rng = np.random.default_rng(7)
    M, K = _camera(rng, 3, plain=False)
    u = rng.random((3, 17 * 9, 4)).astype(F)
    clean = [N_(t) for t in native.camera_rays(T(M), T(K), (17, 9), None, 4, 0.88, 1.12, T(u))]
    M2, K2 = M.copy(), K.copy()
    M2[1, 0, 1] = np.nan
    K2[1, 2] = np.nan
    got = [N_(t) for t in native.camera_rays(T(M2), T(K2), (17, 9), None, 4, 0.88, 1.12, T(u))]
    want = CE.camera_rays(M2, K2, (17, 9), None, 4, 0.88, 1.12, u)
    for name, g, r, c in zip(("origins", "dirs", "z"), got, want, clean):
        _same_bits(name, g, r)
        for b in (0, 2):
            assert np.array_equal(_bits(g[b]), _bits(c[b])), (name, b)
    assert np.isnan(got[1][1]).all() and np.isfinite(got[0][1]).all() and np.isfinite(got[2]).all()


# ---------------------------------------------------------------------------------------------------
# 8. anchor: the reference's camera gives fenerf_ray_setup's bits
# ---------------------------------------------------------------------------------------------------
def _anchor(S, N, fov=12, ray_range=(0.88, 1.12)):
    u = np.random.default_rng(40 + S).random((3, S * S, N)).astype(F)
    z_cam = (-torch.ones(1) / np.tan((2 * math.pi * fov / 360) / 2)).item()
    ref = [N_(t) for t in native.ray_setup(3, S, N, z_cam, ray_range[0], ray_range[1], T(u), T(RC.RAY_THETA), T(RC.RAY_PHI))]
    M = CE.lookat_cam2world(ref[0][:, 0, :])
    K = np.tile(np.array([1, 1, 0, 0, z_cam], dtype=F), (3, 1))
    return u, ref, M, K


@pytest.mark.parametrize("S", [1, 3, 16, 17])
def test_reference_camera_is_ray_setup_bit_for_bit(S):
    N = 5
    u, ref, M, K = _anchor(S, N)
    got = native.camera_rays(T(M), T(K), (S, S), None, N, 0.88, 1.12, T(u))
    for name, g, r in zip(("origins", "dirs", "z"), got, ref[:3]):
        _same_bits(f"{name} S={S}", N_(g), r)


# ---------------------------------------------------------------------------------------------------
# 9. backward kernel against the fp64 terms
# ---------------------------------------------------------------------------------------------------
GRAD_WINDOWS = {1: ((5, 3), (4, 2, 1, 1)), 63: ((17, 9), (3, 1, 9, 7)), 64: ((16, 16), (8, 8, 8, 8)), 65: ((17, 9), (2, 4, 13, 5)),
                257: ((300, 4), (40, 3, 257, 1)), 4097: ((250, 20), (9, 2, 241, 17))}


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("R", sorted(GRAD_WINDOWS))
def test_camera_grads_kernel_vs_fp64_terms(R, B):
    """every one of the 17 sums within (L(R) + 16) 2^-24 sum |terms| of the fp64 sum: L(R) additions on the chain a term travels
    (fenerf_camera_grads_chain_length), 16 for the arithmetic that makes one term; two launches give the same bits; each NULL input
    leaves its outputs exactly zero; the workspace size is honoured and a shorter one refused"""
    size, window = GRAD_WINDOWS[R]
    assert window[2] * window[3] == R
    rng = np.random.default_rng(1000 * B + R)
    M, K = _camera(rng, B, plain=False)
    d_o, d_d = rng.normal(size=(B, R, 3)).astype(F), rng.normal(size=(B, R, 3)).astype(F)
    L = native.camera_grads_chain_length(R)
    assert 0 < L <= 64
    l = _lib.lib()
    nbytes = int(l.fenerf_camera_grads_workspace_bytes(B, R))
    assert nbytes > 0
    # a workspace of exactly the stated size inside a poisoned buffer: nothing beyond it is written
    pad = 256
    buf = torch.full((nbytes + 2 * pad,), 0xA5, dtype=torch.uint8, device=DEV)
    ws = buf[pad:pad + nbytes]
    dM, dK = native.camera_grads(T(M), T(K), size, window, T(d_o), T(d_d), workspace=ws)
    torch.cuda.synchronize()
    assert bool((buf[:pad] == 0xA5).all()) and bool((buf[pad + nbytes:] == 0xA5).all())
    got = np.concatenate([N_(dM).reshape(B, 12), N_(dK)], -1)
    terms = CE.camera_grad_terms(M, K, size, window, d_o, d_d)
    ref, mag = terms.sum(1), np.abs(terms).sum(1)
    err = np.abs(got.astype(np.float64) - ref)
    bound = (L + 16) * EPS24 * mag
    print(f"[camera] grads R={R} B={B} L={L}: worst err / (2^-24 sum|terms|) = {float((err / (EPS24 * mag)).max()):.2f} (bound {L + 16})")
    assert np.isfinite(got).all() and (err <= bound).all(), (err / (EPS24 * mag)).max()
    again = native.camera_grads(T(M), T(K), size, window, T(d_o), T(d_d))
    assert np.array_equal(_bits(N_(again[0])), _bits(N_(dM))) and np.array_equal(_bits(N_(again[1])), _bits(N_(dK)))
    # NULL inputs
    dM_o, dK_o = (N_(t) for t in native.camera_grads(T(M), T(K), size, window, T(d_o), None))
    assert not dM_o[:, :, :3].any() and not dK_o.any() and np.array_equal(_bits(dM_o[:, :, 3]), _bits(N_(dM)[:, :, 3]))
    dM_d, dK_d = (N_(t) for t in native.camera_grads(T(M), T(K), size, window, None, T(d_d)))
    assert not dM_d[:, :, 3].any() and np.array_equal(_bits(dM_d[:, :, :3]), _bits(N_(dM)[:, :, :3])) and np.array_equal(_bits(dK_d), _bits(N_(dK)))
    # a short workspace
    with pytest.raises(_lib.FenerfError) as e:
        native.camera_grads(T(M), T(K), size, window, T(d_o), T(d_d), workspace=buf[:nbytes - 1])
    assert e.value.code == _lib.E_INVALID and "workspace" in str(e.value)


# ---------------------------------------------------------------------------------------------------
# 10. refusals
# ---------------------------------------------------------------------------------------------------
def test_c_abi_refusals():
    l = _lib.lib()
    B, W, H, N = 2, 6, 4, 3
    rng = np.random.default_rng(3)
    M, K = (T(a) for a in _camera(rng, B, plain=True))
    u = T(rng.random((B, W * H, N)).astype(F))
    o, d, g = (torch.zeros((B, W * H, 3), device=DEV) for _ in range(3))
    z = torch.zeros((B, W * H, N), device=DEV)
    dM, dK = torch.zeros((B, 3, 4), device=DEV), torch.zeros((B, 5), device=DEV)
    ws = torch.empty(int(l.fenerf_camera_grads_workspace_bytes(B, W * H)), dtype=torch.uint8, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())

    def rays(win=(0, 0, W, H), n=N, ptrs=None):
        ptrs = ptrs or [p(M), p(K), p(u), p(o), p(d), p(z)]
        return l.fenerf_camera_rays(B, W, H, *win, n, ptrs[0], ptrs[1], 0.88, 1.12, ptrs[2], ptrs[3], ptrs[4], ptrs[5], None)

    def grads(win=(0, 0, W, H), ptrs=None, nbytes=None):
        ptrs = ptrs or [p(M), p(K), p(g), p(g), p(dM), p(dK), p(ws)]
        return l.fenerf_camera_grads(B, W, H, *win, *ptrs[:6], ptrs[6], ws.numel() if nbytes is None else nbytes, None)

    def refused(rc, word):
        msg = l.fenerf_last_error().decode()
        assert rc == _lib.E_INVALID and msg and word in msg, (rc, msg)

    for win in ((-1, 0, 2, 2), (0, -1, 2, 2), (5, 0, 2, 2), (0, 3, 2, 2), (0, 0, W + 1, 1), (0, 0, -1, 2), (2 ** 31 - 1, 0, 2, 2)):
        refused(rays(win), "outside")
        refused(grads(win), "outside")
    for win in ((0, 0, 0, 2), (3, 2, 2, 0), (W, H, 0, 0)):
        refused(rays(win), "no pixel")
        refused(grads(win), "no pixel")
    for n in (0, -3):
        refused(rays(n=n), "N >= 1")
    full = [p(M), p(K), p(u), p(o), p(d), p(z)]
    for i in range(6):
        refused(rays(ptrs=full[:i] + [None] + full[i + 1:]), "NULL")
    full = [p(M), p(K), p(g), p(g), p(dM), p(dK), p(ws)]
    for i in (0, 1, 4, 5):
        refused(grads(ptrs=full[:i] + [None] + full[i + 1:]), "NULL")
    refused(grads(ptrs=full[:6] + [None]), "workspace")
    refused(grads(nbytes=ws.numel() - 1), "workspace")
    assert l.fenerf_camera_grads_workspace_bytes(0, 5) == 0 and l.fenerf_camera_grads_workspace_bytes(1, 0) == 0
    # and the accepted calls: both gradient inputs NULL is a (zero) answer, not an error
    assert rays() == _lib.OK and grads() == _lib.OK
    assert grads(ptrs=full[:2] + [None, None] + full[4:]) == _lib.OK
    torch.cuda.synchronize()
    assert not dM.any() and not dK.any()


# ---------------------------------------------------------------------------------------------------
# 11 - 13. end to end through the generator
# ---------------------------------------------------------------------------------------------------
def _tiny_generator():
    gen = callers.load_generator(os.path.join(GOLDEN, "ref_generator_tiny.pth"), DEV, use_ema=False)
    for p_ in gen.parameters():
        p_.requires_grad_(False)
    gen.siren.sparse_backward = gen.siren.split_backward = False       # the dense one-node render, whatever the ray count
    torch.manual_seed(5)
    zg, za = callers._latent_dims(gen)
    with torch.no_grad():
        fg, pg = gen.siren.geo_mapping_network(torch.randn(1, zg, device=DEV))
        fa, pa = gen.siren.app_mapping_network(torch.randn(1, za, device=DEV))
    return gen, (fg, fa, pg, pa)             # the order forward_with_frequencies takes them in


def _draws(rng, R, N, hierarchical=True):
    """the draws of one render in their order, as [1, R, ...] arrays a window can be cut from: jitter, coarse noise, u, final noise"""
    d = dict(jitter=rng.random((1, R, N, 1)), noise_f=rng.normal(size=(1, R, 2 * N if hierarchical else N, 1)))
    if hierarchical:
        d.update(noise_c=rng.normal(size=(1, R, N, 1)), u=rng.random((1, R, N)))
    return {k: v.astype(F) for k, v in d.items()}


def _recorded(d, rows=None):
    take = lambda a: a if rows is None else np.ascontiguousarray(a[:, rows])
    seq = [take(d["jitter"])]
    if "u" in d:
        seq += [take(d["noise_c"]), take(d["u"]).reshape(-1, d["u"].shape[-1])]
    return VR.RecordedDraws(seq + [take(d["noise_f"])])


RENDER_KW = dict(ray_start=0.88, ray_end=1.12, hierarchical_sample=True, clamp_mode="relu", nerf_noise=0.3, last_back=False)


def test_forward_camera_is_forward_at_the_same_angles():
    gen, film = _tiny_generator()
    S, N = 16, 6
    u, ref, M, K = _anchor(S, N)
    d = _draws(np.random.default_rng(11), S * S, N)
    b = 1                                          # the pose inside the pitch clamp
    with torch.no_grad():
        gen.draws = _recorded(d)
        px_a, poses, depth_a = gen.forward_with_frequencies(*film, img_size=S, fov=12, num_steps=N, h_stddev=0, v_stddev=0,
                                                            h_mean=float(RC.RAY_THETA[b]), v_mean=float(RC.RAY_PHI[b]), sample_dist=None,
                                                            return_depth=True, **RENDER_KW)
        cam = Camera(T(M[b:b + 1]), T(K[b:b + 1]), (S, S))
        gen.draws = _recorded(d)
        px_c, m_out, depth_c = gen.forward_camera_with_frequencies(*film, cam, num_steps=N, return_depth=True, **RENDER_KW)
        assert not gen.draws.arrays, "the camera route makes the angle route's draws, no more"
    assert px_c.shape == (1, gen.output_dim - 1, S, S) and depth_c.shape == (1, S, S) and m_out is cam.cam2world
    _same_bits("pixels", N_(px_c), N_(px_a))
    _same_bits("depth", N_(depth_c), N_(depth_a))
    # Camera.from_angles is that camera too (torch's sin / cos on the device against the kernel's: values, not bits)
    auto = Camera.from_angles(float(RC.RAY_THETA[b]), float(RC.RAY_PHI[b]), 12, (S, S), device=DEV)
    np.testing.assert_allclose(N_(auto.cam2world), M[b:b + 1], atol=1e-6)
    _same_bits("intrinsics", N_(auto.intrinsics), K[b:b + 1])


def test_forward_camera_non_square_frame():
    gen, film = _tiny_generator()
    W, H, N = 20, 12, 6
    R = W * H
    rng = np.random.default_rng(12)
    cam = Camera.from_angles(1.4, 1.7, 14, (W, H), radius=1.05, roll=0.3, device=DEV)
    d = _draws(rng, R, N)
    with torch.no_grad():
        gen.draws = _recorded(d)
        px, _, depth = gen.forward_camera_with_frequencies(*film, cam, num_steps=N, return_depth=True, **RENDER_KW)
        assert px.shape == (1, gen.output_dim - 1, H, W) and depth.shape == (1, H, W)      # forward's channels: no fill mode
        o, dd, z = native.camera_rays(cam.cam2world, cam.intrinsics, (W, H), None, N, 0.88, 1.12, T(d["jitter"]))
        fg, fa, pg, pa = film
        opts = _lib.composite_opts("relu", 0.3)
        rgb, dep, _, _ = gen.siren.native(DEV).render(o, dd, z, T(d["u"]).reshape(R, N), T(d["noise_c"]).reshape(1, R, N),
                                                      T(d["noise_f"]).reshape(1, R, 2 * N), fg, pg, fa, pa, opts, hierarchical=True, lock_view=False)
    want = rgb.reshape(1, H, W, -1).permute(0, 3, 1, 2).contiguous() * 2 - 1
    _same_bits("pixels", N_(px), N_(want))
    _same_bits("depth", N_(depth), N_(dep.reshape(1, H, W)))
    # a staged render of the same camera with the inversion previews' fill mode: [1, 22, 12, 20] (the background channel joins), on the CPU
    with torch.no_grad():
        gen.draws = _recorded(d)
        img, depth_map, third = gen.staged_forward_camera_with_frequencies(*film, cam, num_steps=N, fill_mode="eval_seg_padding_background",
                                                                           fill_color="black", **RENDER_KW)
    assert img.shape == (1, 22, H, W) and gen.output_dim == 22 and depth_map.shape == (1, H, W) and not img.is_cuda
    assert third.shape[0] == 1 and third.shape[2:] == (H, W)
    _same_bits("staged depth", depth_map.numpy(), N_(depth))


def test_tiles_stitch_to_the_full_frame():
    """four 8 x 8 windows of a 16 x 16 frame, each with its slice of the frame's draws: the frame's pixels and depth, bit for bit"""
    gen, film = _tiny_generator()
    S, N = 16, 6
    kw = dict(RENDER_KW, nerf_noise=0)
    cam = Camera.from_angles(1.45, 1.65, 12, (S, S), roll=-0.2, device=DEV)
    d = _draws(np.random.default_rng(13), S * S, N)
    with torch.no_grad():
        gen.draws = _recorded(d)
        full, _, depth = gen.forward_camera_with_frequencies(*film, cam, num_steps=N, return_depth=True, **kw)
        stitched, stitched_depth = torch.zeros_like(full), torch.zeros_like(depth)
        for x0, y0 in ((0, 0), (8, 0), (0, 8), (8, 8)):
            rows = (np.arange(y0, y0 + 8)[:, None] * S + np.arange(x0, x0 + 8)[None]).reshape(-1)
            gen.draws = _recorded(d, rows)
            px, _, dep = gen.forward_camera_with_frequencies(*film, cam.crop(x0, y0, 8, 8), num_steps=N, return_depth=True, **kw)
            assert px.shape == (1, gen.output_dim - 1, 8, 8)
            stitched[:, :, y0:y0 + 8, x0:x0 + 8] = px
            stitched_depth[:, y0:y0 + 8, x0:x0 + 8] = dep
    _same_bits("pixels", N_(stitched), N_(full))
    _same_bits("depth", N_(stitched_depth), N_(depth))


def test_camera_gradients_end_to_end():
    gen, film = _tiny_generator()
    S, N = 8, 4
    R = S * S
    d = _draws(np.random.default_rng(14), R, N)
    base = Camera.from_angles(1.5, 1.62, 12, (S, S), roll=0.1, device=DEV)
    M0 = N_(base.cam2world)
    K0 = N_(base.intrinsics) + np.array([[0.1, -0.05, 0.02, -0.03, 0.0]], dtype=F)

    def run(camera_grad):
        cam = Camera(T(M0).requires_grad_(camera_grad), T(K0).requires_grad_(camera_grad), (S, S))
        f = [t.clone().requires_grad_() for t in film]
        rays = {}
        gen.draws = _recorded(d)
        px, _, depth = gen.forward_camera_with_frequencies(*f, cam, num_steps=N, return_depth=True, rays_out=rays, **RENDER_KW)
        if camera_grad:
            rays["origins"].retain_grad()
            rays["dirs"].retain_grad()
        ((px ** 2).mean() + depth.mean()).backward()
        return cam, f, rays, px

    cam, f, rays, px = run(True)
    _, f0, rays0, px0 = run(False)
    _same_bits("pixels", N_(px), N_(px0))
    assert not rays0["origins"].requires_grad and rays["dirs"].requires_grad
    for a, b in zip(f, f0):
        _same_bits("FiLM gradient", N_(a.grad), N_(b.grad))
    d_o, d_d = N_(rays["origins"].grad), N_(rays["dirs"].grad)
    assert np.abs(d_d).max() > 0 and np.abs(d_o).max() > 0
    terms = CE.camera_grad_terms(M0, K0, (S, S), None, d_o, d_d)
    ref, mag = terms.sum(1), np.abs(terms).sum(1)
    got = np.concatenate([N_(cam.cam2world.grad).reshape(1, 12), N_(cam.intrinsics.grad)], -1).astype(np.float64)
    L = native.camera_grads_chain_length(R)
    assert (np.abs(got - ref) <= (L + 16) * EPS24 * mag).all(), (np.abs(got - ref) / (EPS24 * mag)).max()
    assert np.abs(got).min() > 0
    # the sparse and the two-node renders refuse a camera that requires grad as they refuse an h_mean tensor
    for p_ in gen.parameters():
        p_.requires_grad_(True)
    try:
        for attr in ("sparse_backward", "split_backward"):
            setattr(gen.siren, attr, True)
            errors = []
            for route in ("camera", "angles"):
                gen.draws = _recorded(d)
                with pytest.raises(NotImplementedError) as e:
                    if route == "camera":
                        c = Camera(T(M0).requires_grad_(), T(K0), (S, S))
                        gen.forward_camera_with_frequencies(*film, c, num_steps=N, **RENDER_KW)
                    else:
                        gen.forward_with_frequencies(*film, img_size=S, fov=12, num_steps=N, h_stddev=0, v_stddev=0, sample_dist=None,
                                                     h_mean=torch.tensor(1.5, device=DEV, requires_grad=True), v_mean=1.62, **RENDER_KW)
                errors.append(str(e.value))
            assert errors[0] == errors[1] and "rays" in errors[0], errors
            setattr(gen.siren, attr, False)
    finally:
        gen.siren.sparse_backward = gen.siren.split_backward = False


# ---------------------------------------------------------------------------------------------------
# 14. callers.inverse_render(pose_model="se3")
# ---------------------------------------------------------------------------------------------------
def test_inverse_render_se3():
    torch.manual_seed(7)
    mod, spec, sd = _siren_module("texture", 32, 5, sigma_gain=150.0)
    gen = _double_generator(mod).eval()
    for p_ in gen.parameters():
        p_.requires_grad_(False)
    gen.draws = _FixedDraws()
    hv = math.pi / 2
    S = 16
    opts = dict(img_size=S, fov=12, ray_start=0.88, ray_end=1.12, num_steps=12, h_stddev=0, v_stddev=0, h_mean=torch.tensor(hv, device=DEV),
                v_mean=torch.tensor(hv, device=DEV), hierarchical_sample=False, sample_dist=None, clamp_mode="relu", nerf_noise=0, last_back=False)
    rotvec, shift = torch.tensor([[0.01, -0.02, 0.03]], device=DEV), torch.tensor([[0.004, 0.0, -0.006]], device=DEV)
    with torch.no_grad():       # the FiLM state inverse_render starts from (init_psi = 0, zero draws: the mapping of the zero latent)
        fg, pg = gen.siren.geo_mapping_network(torch.zeros(1, 8, device=DEV))
        fa, pa = gen.siren.app_mapping_network(torch.zeros(1, 8, device=DEV))
        true_cam = Camera.from_angles(hv, hv, 12, (S, S), device=DEV).perturbed(rotvec, shift)
        target = gen.forward_camera_with_frequencies(fg, fa, pg, pa, true_cam, 0.88, 1.12, 12, False, clamp_mode="relu", nerf_noise=0, last_back=False)[0]
    seen = []
    res = callers.inverse_render(gen, target[:, -3:], target[:, :-3], opts, n_iterations=40, z_dim=8, latent_noise=0.0, n_mean_latents=4, lr=0.0,
                                 lr_pose=5e-4, optimize_pose=True, pose_model="se3", on_step=lambda i, loss, meta: seen.append(meta))
    losses = res["losses"]
    print(f"[camera] inverse_render(se3), 40 iterations: loss {losses[0]:.4e} -> {losses[-1]:.4e}")
    assert len(losses) == 40 and np.isfinite(losses).all() and losses[-1] < losses[0]
    assert res["cam2world"].shape == (1, 3, 4) and res["intrinsics"].shape == (1, 5)
    assert bool(torch.isfinite(res["cam2world"]).all()) and bool(torch.isfinite(res["intrinsics"]).all())
    assert not res["cam2world"].requires_grad and not torch.equal(res["cam2world"], Camera.from_angles(hv, hv, 12, (S, S), device=DEV).cam2world)
    assert len(seen) == 40 and all("cam2world" in m and "intrinsics" in m for m in seen)
    for k in res:
        if "offset" in k and k != "offset_history":
            assert not res[k].any(), "lr = 0: the FiLM state stays the target's"
    # the focal length joins the group on request
    foc = callers.inverse_render(gen, target[:, -3:], target[:, :-3], opts, n_iterations=3, z_dim=8, latent_noise=0.0, n_mean_latents=4, lr=0.0,
                                 lr_pose=5e-4, optimize_pose=True, pose_model="se3", optimize_focal=True)
    assert foc["intrinsics"][0, 0] != 1 and foc["intrinsics"][0, 0] == foc["intrinsics"][0, 1] and foc["intrinsics"][0, 4] == res["intrinsics"][0, 4]
    # pose_model="angles" is the optimize_pose of the previous signature, bit for bit
    kw = dict(n_iterations=5, z_dim=8, latent_noise=0.0, n_mean_latents=4, optimize_pose=True)
    a = callers.inverse_render(gen, target[:, -3:], target[:, :-3], opts, **kw)
    b = callers.inverse_render(gen, target[:, -3:], target[:, :-3], opts, pose_model="angles", **kw)
    assert a["losses"] == b["losses"] and a["yaw"] == b["yaw"] and a["pitch"] == b["pitch"] and "cam2world" not in b
    for k in a:
        if "offset" in k:
            assert torch.equal(a[k], b[k]), k


# ---------------------------------------------------------------------------------------------------
# every camera entry of every generator class against the angle entry it stands beside
# ---------------------------------------------------------------------------------------------------
def _single_latent(cls):
    torch.manual_seed(9)                       # the module is torch-initialised
    gen = cls(functools.partial(S.SPATIALSIRENBASELINE, hidden_dim=32), 16, 4).to(DEV)
    gen.set_device(torch.device(DEV))
    return gen.eval()


def _class_cases(kind):
    """-> (generator, {entry name: positional arguments}, the staged entries' extra kwargs)"""
    torch.manual_seed(31)
    if kind == "double":
        gen, film = _tiny_generator()
        z = (torch.randn(1, 16, device=DEV), torch.randn(1, 16, device=DEV))
        return gen, dict(forward=z, forward_with_frequencies=film, staged_forward=z, staged_forward_with_frequencies=film), \
            dict(psi=0.7, fill_mode="eval_seg_padding_background", fill_color="black")
    gen = _single_latent(G.ImplicitGenerator3d if kind == "single" else G.StyleGenerator3d)
    z = (torch.randn(1, 16, device=DEV),)
    with torch.no_grad():
        film = tuple(gen.siren.mapping_network(torch.randn(1, 16, device=DEV)))
    return gen, dict(forward=z, forward_with_frequencies=film, staged_forward=z, staged_forward_with_frequencies=film), \
        dict(psi=0.7, fill_mode="weight", fill_color="white")


@pytest.mark.parametrize("kind", ["double", "single", "style"])
def test_every_camera_entry_is_its_angle_entry(kind):
    """forward, forward_with_frequencies, staged_forward and staged_forward_with_frequencies of the three generator classes at a fixed pose
    against their *_camera forms with that pose's camera, from the same generator seed: every returned tensor bit for bit (the poses,
    which the camera entries replace by cam2world, aside) -- pixels under a fill mode, depth maps and the third staged output included"""
    gen, entries, staged_kw = _class_cases(kind)
    S_, N, b = 16, 4, 1
    _, _, M, K = _anchor(S_, N)
    cam = Camera(T(M[b:b + 1]), T(K[b:b + 1]), (S_, S_))
    shared = dict(ray_start=0.88, ray_end=1.12, num_steps=N, hierarchical_sample=True, clamp_mode="relu", nerf_noise=0.3, last_back=False)
    angles = dict(img_size=S_, fov=12, h_stddev=0, v_stddev=0, h_mean=float(RC.RAY_THETA[b]), v_mean=float(RC.RAY_PHI[b]), sample_dist=None)
    for name, args in entries.items():
        kw = dict(shared, **(staged_kw if name.startswith("staged") else dict(return_depth=True)))
        with torch.no_grad():
            torch.manual_seed(77)
            want = getattr(gen, name)(*args, **angles, **kw)
            torch.manual_seed(77)
            got = getattr(gen, name.replace("forward", "forward_camera", 1))(*args, cam, **kw)
            after = (float(torch.rand(1, device=DEV)), float(torch.rand(1)))
            torch.manual_seed(77)
            getattr(gen, name)(*args, **angles, **kw)
            assert after == (float(torch.rand(1, device=DEV)), float(torch.rand(1))), f"{kind} {name}: the camera entry consumes the generator as the angle entry"
        assert len(got) == len(want) and len(got) >= 2, (kind, name)
        for i, (g, w) in enumerate(zip(got, want)):
            if i == 1 and not name.startswith("staged"):
                assert g is cam.cam2world
                continue
            assert g.is_cuda == w.is_cuda, (kind, name, i)
            _same_bits(f"{kind} {name} output {i}", N_(g), N_(w))


# ---------------------------------------------------------------------------------------------------
# callers.render_multiview(cameras=...) and the tool's flags behind the parser
# ---------------------------------------------------------------------------------------------------
def test_render_multiview_with_cameras():
    gen, _ = _tiny_generator()
    g = load_golden("tiny_multiview")
    cur = {(int(k[4:]) if k.startswith("int:") else k): v for k, v in json.loads(str(g["curriculum_json"])).items()}
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import render_multiview as tool
    finally:
        sys.path.pop(0)
    opt = tool.parse_options(["g.pth", "--image_size", "16", "--roll", "20", "--radius", "1.1", "--crop", "4", "2", "8", "10"])
    cams = tool.view_cameras(opt, cur, DEV)
    assert len(cams) == 5 and all(c.window == (4, 2, 8, 10) and c.size == (16, 16) and c.frame == (8, 10) for c in cams)
    plain = Camera.from_angles(tool.FACE_ANGLES[0] + cur["h_mean"], cur["v_mean"], cur["fov"], (16, 16), device=DEV)
    np.testing.assert_allclose(N_(cams[0].cam2world[:, :, 3]), 1.1 * N_(plain.cam2world[:, :, 3]), rtol=1e-6)
    a = math.radians(20)
    np.testing.assert_allclose(N_(cams[0].cam2world[:, :, 0]), N_(math.cos(a) * plain.cam2world[:, :, 0] + math.sin(a) * plain.cam2world[:, :, 1]), atol=1e-6)
    # two cameras with frames of one size: a window of a 16 x 16 image and a whole 8 x 10 image
    two = [cams[1], Camera.from_angles(1.3, 1.6, 14, (8, 10), roll=-0.3, device=DEV)]
    seed, mult = 3, 1
    images, segmaps = callers.render_multiview(gen, cur, seed, DEV, ray_step_multiplier=mult, cameras=two)
    assert images.shape == (2, 3, 10, 8) and segmaps.shape == (2, 3, 10, 8) and not images.is_cuda
    kw = {k: v for k, v in callers.multiview_kwargs(cur, 256, mult, False).items() if k not in callers._ANGLE_CAMERA_KEYS}
    zg, za = callers._latent_dims(gen)
    for i, cam in enumerate(two):
        torch.manual_seed(seed)
        z_geo, z_app = torch.randn((1, zg), device=DEV), torch.randn((1, za), device=DEV)
        img, depth_map = gen.staged_forward_camera(z_geo, z_app, cam, **kw)
        assert depth_map.shape == (1, 10, 8)
        _same_bits(f"view {i} rgb", N_(images[i:i + 1]), N_(img[:, -3:]))
        _same_bits(f"view {i} labels", N_(segmaps[i:i + 1]), N_(callers.mask2color(img[:, :-3], DEV, scale=255.0)))
    assert not torch.equal(images[0], images[1])
    with pytest.raises(ValueError, match="empty"):
        callers.render_multiview(gen, cur, seed, DEV, cameras=[])
