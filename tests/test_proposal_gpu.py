"""The proposal lattice on the device: fenerf_proposal_depths against the chain of public calls it stands for, fenerf_render_proposal
against its three public calls, every refusal of the header, the Python route (bake_density -> DensityField.render -> render_multiview) and
the route's fidelity against the exact render's own Monte-Carlo spread."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from test_volume_gpu import DEV, N_, OPTS, OUT, T, _bits, _frame, _rays, _siren_module, _tiny_generator, proc
from fenerf_amd import _lib, callers, native
from fenerf_amd.generators import volumetric_rendering as VR

pytestmark = pytest.mark.gpu


def _t_of(x, origin, spacing):
    return np.float32(np.float32(x - np.float32(origin)) / np.float32(spacing))


def _last_plane_coordinate(n, origin, spacing):
    """the largest fp32 coordinate the inside test accepts on an axis of n points: t == n - 1 exactly"""
    x = np.float32(np.float32(origin) + np.float32(n - 1) * np.float32(spacing))
    while _t_of(x, origin, spacing) > np.float32(n - 1):
        x = np.nextafter(x, np.float32(-np.inf))
    while _t_of(np.nextafter(x, np.float32(np.inf)), origin, spacing) <= np.float32(n - 1):
        x = np.nextafter(x, np.float32(np.inf))
    assert _t_of(x, origin, spacing) == np.float32(n - 1)
    return x


def _kernel_arrays(shape, R, N):
    """rays of test_volume_gpu._rays (most leave the lattice midway) with, in image 0: ray 0 wholly outside the lattice, ray 1 with one NaN
    depth, ray 2 on the last plane of axis 0; a density lattice of both signs"""
    B = 2
    origin, spacing = _frame(shape)
    vol = (np.random.default_rng(11).uniform(-1, 1, shape) * 40.0).astype(np.float32)
    o, d, z = _rays(B, R, N, seed=7)
    o[0, 0] = (0.0, 0.0, 5.0)
    z[0, 1, 1] = np.nan
    o[0, 2] = (_last_plane_coordinate(shape[0], origin[0], spacing[0]), 0.01, 0.45)
    d[0, 2] = (0.0, 0.0, -1.0)
    rng = np.random.default_rng(12)
    u = rng.uniform(0, 1, (B * R, N)).astype(np.float32)
    nc = rng.normal(size=(B, R, N)).astype(np.float32)
    return origin, spacing, vol, o, d, z, u, nc


@functools.lru_cache(maxsize=None)
def _kernel_case(shape, R, N):
    origin, spacing, *arrays = _kernel_arrays(shape, R, N)
    return (origin, spacing) + tuple(T(a) for a in arrays)


def _chain(vol, origin, spacing, o, d, z, u, noise_c, copts):
    """volume_sample_rays (C = 1) -> composite on rows [0 | sigma] -> resample -> torch.sort (stable, NaN last) -> (z_fine, w, sigma)"""
    B, R, N = z.shape
    sigma = native.volume_sample_rays(vol.unsqueeze(-1), origin, spacing, o, d, z, OUT, 1)
    rows = torch.cat([torch.zeros_like(sigma), sigma], dim=-1)
    w = native.composite(rows, z, noise_c, copts, want_wsum=False)[2]
    zf = native.resample(z.reshape(B * R, N), w.reshape(B * R, N), u)
    zs = torch.sort(zf.cpu(), dim=-1, stable=True).values
    return N_(zs).reshape(B, R, N), N_(w), N_(sigma)[..., 0]


@pytest.mark.parametrize("N", [3, 12, 65, 512])
@pytest.mark.parametrize("R", [16, 3])
@pytest.mark.parametrize("shape", [(5, 4, 3), (8, 8, 8)])
def test_kernel_equals_the_chain_of_public_calls_bit_for_bit(shape, R, N):
    origin, spacing, vol, o, d, z, u, nc = _kernel_case(shape, R, N)
    for clamp in ("relu", "softplus"):
        for noise_std in (0.0, 0.7):
            copts = _lib.composite_opts(clamp, noise_std)
            noise_c = nc if noise_std else None
            zf, w = native.proposal_depths(vol, origin, spacing, o, d, z, u, noise_c, copts, OUT, want_weights=True)
            assert zf.shape == w.shape == z.shape and zf.dtype == torch.float32 and zf.is_cuda
            want_zf, want_w, sigma = _chain(vol, origin, spacing, o, d, z, u, noise_c, copts)
            got_zf, got_w = N_(zf), N_(w)
            for name, a, b in (("z_fine", got_zf, want_zf), ("coarse_weights", got_w, want_w)):
                differ = _bits(a) != _bits(b)
                assert not differ.any(), (clamp, noise_std, name, int(differ.sum()), a.size)
            zf_only, none = native.proposal_depths(vol, origin, spacing, o, d, z, u, noise_c, copts, OUT)          # coarse_weights NULL: not written
            assert none is None and np.array_equal(_bits(N_(zf_only)), _bits(got_zf))
            # what the case is made of
            inside = sigma != np.float32(OUT)
            assert (sigma[inside] > 0).any() and (sigma[inside] < 0).any()                           # both branches of the clamp
            leaves = inside.any(-1) & ~inside.all(-1)
            assert leaves[1].any()                                                                   # rays that leave the lattice midway
            assert not inside[0, 0].any() and not got_w[0, 0].any()                                  # wholly outside: every weight is 0 ...
            uniform = native.resample(z[0, :1].reshape(1, N), torch.zeros((1, N), device=DEV), u[:1])
            assert np.array_equal(_bits(got_zf[0, 0]), _bits(np.sort(N_(uniform)[0])))               # ... and the depths are the uniform pdf's
            assert inside[0, 2].any()                                                                # the ray on the last plane reads the lattice
            nan = np.isnan(got_zf)
            assert nan[0, 1].any() and not np.delete(nan.reshape(-1, N), 1, axis=0).any()            # the NaN stays in its own ray ...
            k = int(nan[0, 1].sum())
            assert nan[0, 1, N - k:].all() and not nan[0, 1, :N - k].any()                           # ... and sorts last
            rest = np.where(nan, np.float32(3e38), got_zf)
            assert (np.diff(rest, axis=-1) >= 0).all()                                               # ascending


@functools.lru_cache(maxsize=None)
def _render_case():
    """the tiny texture SIREN, B = 2 cameras of 4 x 4 rays with 12 samples, an 8^3 density lattice of both signs around the origin"""
    mod, spec, sd = _siren_module("texture", 32, 6, sigma_gain=150.0)
    nat = mod.native(torch.device(DEV))
    B, S_, N = 2, 4, 12
    film = tuple(T(proc.film_params(spec, B, seed=4)[k]) for k in ("freq_geo", "phase_geo", "freq_app", "phase_app"))
    shape = (8, 8, 8)
    origin, spacing = _frame(shape)
    vol = T((np.random.default_rng(21).uniform(-1, 1, shape) * 40.0).astype(np.float32))
    torch.manual_seed(3)
    o, d, z, _, _ = VR.sample_rays(B, N, DEV, 12, (S_, S_), 0.88, 1.12, 0.3, 0.155, math.pi / 2, math.pi / 2, "gaussian")
    rng = np.random.default_rng(22)
    R = S_ * S_
    u, nc, nf = T(rng.uniform(0, 1, (B * R, N))), T(rng.normal(size=(B, R, N))), T(rng.normal(size=(B, R, N)))
    return mod, nat, film, shape, origin, spacing, vol, o.contiguous(), d.contiguous(), z.reshape(B, R, N).contiguous(), u, nc, nf


@pytest.mark.parametrize("kind", sorted(OPTS))
def test_render_equals_its_three_public_calls_bit_for_bit(kind):
    mod, nat, film, shape, origin, spacing, vol, o, d, z, u, nc, nf = _render_case()
    B, R, N = z.shape
    assert l_size(B, R, N, nat.C) > 0
    for noise_std in (0.0, 0.7):
        opts = _lib.composite_opts(noise_std=noise_std, **OPTS[kind])
        noise_c, noise_f = (nc, nf) if noise_std else (None, None)
        pixels = {}
        for lock_view in (False, True):
            got = nat.render_proposal(vol, origin, spacing, o, d, z, u, noise_c, noise_f, *film, opts, outside_last=OUT, lock_view=lock_view,
                                      want_weights=True, want_wsum=True)
            zf, _ = native.proposal_depths(vol, origin, spacing, o, d, z, u, noise_c, opts, OUT)
            rows = nat.siren_forward_rays(o, d, zf, *film, lock_view=lock_view)
            want = native.composite(rows, zf, noise_f, opts)
            for name, a, b in zip(("rgb", "depth", "weights", "wsum"), got, want):
                a, b = N_(a).reshape(-1), N_(b).reshape(-1)
                assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), (kind, noise_std, lock_view, name, float(np.abs(a - b).max()))
            assert tuple(got[2].shape) == (B, R, N) and np.isfinite(N_(got[0])).all()
            assert int((got[3] > 1e-3).sum()) >= 4                                                   # several rays meet matter: the pixels are not all background
            pixels[lock_view] = N_(got[0])
        assert not np.array_equal(pixels[False][..., -3:], pixels[True][..., -3:])                   # the view direction reaches the colour
        assert np.array_equal(_bits(pixels[False][..., :-3]), _bits(pixels[True][..., :-3]))         # ... and nothing else


def l_size(B, R, N, C_):
    return _lib.lib().fenerf_render_proposal_workspace_bytes(B, R, N, C_)


def test_refusals():
    """every refusal include/fenerf.h lists for the two entries, one fault at a time: FENERF_E_INVALID with a message, before anything is launched"""
    mod, nat, film, shape, origin, spacing, vol, o, d, z, u, nc, nf = _render_case()
    B, R, N = z.shape
    l = _lib.lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    f3 = lambda *v: (C.c_float * 3)(*v)
    fg, pg, fa, pa = nat._film(B, *film)
    nbytes = l_size(B, R, N, nat.C)
    keep = dict(ws=torch.empty(nbytes, dtype=torch.uint8, device=DEV), film=torch.empty(l.fenerf_film_workspace_bytes(nat._h, B), dtype=torch.uint8, device=DEV),
                rgb=torch.empty((B, R, nat.C - 1), device=DEV), depth=torch.empty((B, R), device=DEV), w=torch.empty((B, R, N), device=DEV),
                wsum=torch.empty((B, R), device=DEV), zf=torch.empty((B, R, N), device=DEV), opts=_lib.composite_opts("relu", 0.5))
    lat = dict(vol=p(vol), n0=shape[0], n1=shape[1], n2=shape[2], origin=f3(*origin), spacing=f3(*spacing), outside_last=OUT)
    rays = dict(origins=p(o), dirs=p(d), z_coarse=p(z), u=p(u), noise_coarse=p(nc))
    kgood = dict(lat, B=B, R=R, N=N, **rays, opts=C.byref(keep["opts"]), z_fine=p(keep["zf"]), coarse_weights=p(keep["w"]), stream=None)
    rgood = dict(m=nat._h, **lat, B=B, R=R, N=N, lock_view=0, **rays, noise_final=p(nf), freq_geo=p(fg), phase_geo=p(pg), freq_app=p(fa), phase_app=p(pa),
                 opts=C.byref(keep["opts"]), out_rgb=p(keep["rgb"]), out_depth=p(keep["depth"]), out_weights=p(keep["w"]), out_wsum=p(keep["wsum"]),
                 film_ws=p(keep["film"]), workspace=p(keep["ws"]), workspace_bytes=nbytes, stream=None)
    assert l.fenerf_proposal_depths(*kgood.values()) == _lib.OK and l.fenerf_render_proposal(*rgood.values()) == _lib.OK
    torch.cuda.synchronize()
    shared = [(dict(vol=None), "NULL"), (dict(origin=None), "NULL"), (dict(spacing=None), "NULL"), (dict(origins=None), "NULL"), (dict(dirs=None), "NULL"),
              (dict(z_coarse=None), "NULL"), (dict(u=None), "NULL"), (dict(opts=None), "opts is NULL"),
              (dict(n0=1), "at least 2 points"), (dict(n1=1), "at least 2 points"), (dict(n2=1), "at least 2 points"),
              (dict(n0=2048, n1=2048, n2=2048), "2^31 - 1"),
              (dict(spacing=f3(0.0, 0.1, 0.1)), "finite and positive"), (dict(spacing=f3(0.1, -0.1, 0.1)), "finite and positive"),
              (dict(spacing=f3(0.1, 0.1, float("inf"))), "finite and positive"), (dict(spacing=f3(float("nan"), 0.1, 0.1)), "finite and positive"),
              (dict(B=-1), "negative count"), (dict(R=-1), "negative count"),
              (dict(N=2), "3 to 512"), (dict(N=513), "3 to 512"), (dict(N=0), "3 to 512"), (dict(N=-1), "3 to 512")]
    own = [(l.fenerf_proposal_depths, kgood, [(dict(z_fine=None), "NULL")]),
           (l.fenerf_render_proposal, rgood, [(dict(m=None), "NULL"), (dict(out_rgb=None), "NULL"), (dict(freq_geo=None), "NULL"), (dict(phase_geo=None), "NULL"),
                                              (dict(freq_app=None), "NULL"), (dict(phase_app=None), "NULL"), (dict(film_ws=None), "NULL"),
                                              (dict(workspace=None), "workspace too small"), (dict(workspace_bytes=nbytes - 1), "workspace too small")])]
    for fn, good, faults in own:
        for change, text in shared + faults:
            rc = fn(*dict(good, **change).values())
            msg = l.fenerf_last_error().decode()
            assert rc == _lib.E_INVALID and text in msg, (fn.__name__, change, rc, msg)
        assert fn(*dict(good, B=0).values()) == _lib.OK and fn(*dict(good, R=0).values()) == _lib.OK
    bad_clamp = _lib.composite_opts("relu")
    bad_clamp.clamp_mode = 7
    assert l.fenerf_proposal_depths(*dict(kgood, opts=C.byref(bad_clamp)).values()) == _lib.E_CLAMP_MODE
    # optional outputs may be NULL
    assert l.fenerf_proposal_depths(*dict(kgood, coarse_weights=None, noise_coarse=None).values()) == _lib.OK
    assert l.fenerf_render_proposal(*dict(rgood, out_depth=None, out_weights=None, out_wsum=None, noise_coarse=None, noise_final=None).values()) == _lib.OK
    torch.cuda.synchronize()


def _kw(S_, N, **over):
    kw = dict(img_size=S_, fov=12, ray_start=0.88, ray_end=1.12, num_steps=N, h_stddev=0.3, v_stddev=0.155, h_mean=math.pi / 2, v_mean=math.pi / 2,
              hierarchical_sample=True, sample_dist="gaussian", clamp_mode="relu", nerf_noise=0.1, last_back=False,
              fill_mode="eval_seg_padding_background", fill_color="black")
    kw.update(over)
    return kw


def test_python_route_bake_density_render_multiview():
    gen, film, meta = _tiny_generator()
    S_, N = 8, 6
    kw = _kw(S_, N)
    cube = callers.baked_cube_length(kw["fov"], kw["ray_start"], kw["ray_end"], num_steps=N)
    field = callers.bake_density(gen, None, film=meta, resolution=17, cube_length=cube, max_points=17 * 17 * 5)        # several slabs
    assert tuple(field.vol.shape) == (17, 17, 17) and field.vol.is_cuda and field.vol.dtype == torch.float32 and field.outside_last == -1e30
    # the lattice holds the network's own sigma at origin + i * spacing
    nat = gen.siren.native(torch.device(DEV))
    fg, pg, fa, pa = film["freq_geo"], film["phase_geo"], film["freq_app"], film["phase_app"]
    i = torch.tensor([[0, 0, 0], [16, 16, 16], [3, 9, 14]], device=DEV)
    nodes = torch.tensor(field.origin, device=DEV) + i.float() * torch.tensor(field.spacing, device=DEV)
    pts = torch.cat([nodes, nodes[-1:].expand(29, -1)])[None].contiguous()
    held = _bits(N_(field.vol[i[:, 0], i[:, 1], i[:, 2]]))
    assert np.array_equal(held, _bits(N_(nat.siren_forward(pts, None, fg, pg, fa, pa)[0, :3, -1])))
    if nat.supports_density():
        assert np.array_equal(held, _bits(N_(nat.siren_density(pts, fg, pg, labels=False)[0, :3])))
    got = field.sample(nodes)
    assert got.shape == (3,) and got.is_cuda and np.array_equal(_bits(N_(got[:1])), held[:1])      # the first node: t = 0 on every axis, no lerp rounds
    # layout, dtype and device of staged_forward_with_frequencies
    for lock in (False, True):
        torch.manual_seed(5)
        exact = gen.staged_forward_with_frequencies(fg, fa, pg, pa, lock_view_dependence=lock, **kw)
        torch.manual_seed(5)
        prop = field.render(gen, lock_view_dependence=lock, **kw)
        assert len(prop) == len(exact) == 3
        for a, b in zip(prop[:2], exact[:2]):
            assert a.shape == b.shape and a.dtype == b.dtype and a.device == b.device
        assert prop[2].dtype == exact[2].dtype and prop[2].device == exact[2].device and prop[2].shape[0] == exact[2].shape[0] and prop[2].shape[2:] == exact[2].shape[2:]
        assert tuple(prop[0].shape) == (1, 22, S_, S_) and tuple(prop[1].shape) == (1, S_, S_) and torch.isfinite(prop[0]).all()
    # every recorded draw consumed in order; pixels bit for bit those of NativeModel.render_proposal fed the same draws
    R = S_ * S_
    rng = np.random.default_rng(9)
    rec = [rng.uniform(0, 1, (1, R, N, 1)), rng.normal(size=(1, 1)), rng.normal(size=(1, 1)), rng.normal(size=(1, R, N, 1)), rng.uniform(0, 1, (R, N)),
           rng.normal(size=(1, R, 2 * N, 1))]
    rec = [a.astype(np.float32) for a in rec]
    o, d, z, _, _ = VR.sample_rays(1, N, DEV, kw["fov"], (S_, S_), kw["ray_start"], kw["ray_end"], kw["h_stddev"], kw["v_stddev"], kw["h_mean"], kw["v_mean"],
                                   kw["sample_dist"], draws=VR.RecordedDraws(rec[:3]))
    opts = _lib.composite_opts("relu", kw["nerf_noise"], False, False, False, kw["fill_mode"], kw["fill_color"])
    for lock in (False, True):
        gen.draws = VR.RecordedDraws(list(rec))
        try:
            px, depth, _ = field.render(gen, lock_view_dependence=lock, **kw)
            assert not gen.draws.arrays, "all recorded draws consumed, in order"
        finally:
            del gen.draws
        rgb, dep, _, _ = nat.render_proposal(field.vol, field.origin, field.spacing, o, d, z.reshape(1, R, N), T(rec[4]), T(rec[3]).reshape(1, R, N),
                                             T(rec[5]).reshape(1, R, 2 * N)[..., :N].contiguous(), fg, pg, fa, pa, opts, outside_last=field.outside_last,
                                             lock_view=lock)
        want = gen._finish_scaled(rgb, 1, S_)
        assert np.array_equal(_bits(N_(px)), _bits(N_(want))) and np.array_equal(_bits(N_(depth)), _bits(N_(dep.reshape(1, S_, S_))))
    with pytest.raises(ValueError):
        field.render(gen, **dict(kw, hierarchical_sample=False))
    # no-grad only
    g_meta = dict(meta, truncated_frequencies_geo=fg.clone().requires_grad_(True))
    with pytest.raises(RuntimeError):
        callers.bake_density(gen, None, film=g_meta, resolution=5, cube_length=cube)
    g_field = callers.DensityField(field.vol, field.origin, field.spacing, (g_meta["truncated_frequencies_geo"],) + tuple(field.film[1:]))
    with pytest.raises(RuntimeError):
        g_field.render(gen, **kw)
    with pytest.raises(RuntimeError):
        field.render(gen, **dict(kw, h_mean=torch.tensor(math.pi / 2, device=DEV, requires_grad=True)))
    # render_multiview(proposal=17): the layout of the exact call
    cur = {0: dict(num_steps=3, img_size=S_), "fov": 12, "ray_start": 0.88, "ray_end": 1.12, "h_stddev": 0.3, "v_stddev": 0.155, "h_mean": math.pi / 2,
           "v_mean": math.pi / 2, "sample_dist": "gaussian", "clamp_mode": "relu", "hierarchical_sample": True, "fill_mode": "eval_seg_padding_background"}
    angles = (-0.3, 0.0, 0.3)
    ex_img, ex_seg = callers.render_multiview(gen, cur, 1, DEV, face_angles=angles, image_size=S_, z_dim=8)
    pr_img, pr_seg = callers.render_multiview(gen, cur, 1, DEV, face_angles=angles, image_size=S_, z_dim=8, proposal=17)
    assert pr_img.shape == ex_img.shape == (3, 3, S_, S_) and pr_seg.shape == ex_seg.shape and pr_img.dtype == ex_img.dtype and pr_seg.dtype == ex_seg.dtype
    assert pr_img.device == ex_img.device and torch.isfinite(pr_img).all()
    print(f"render_multiview proposal=17 vs exact, 3 views: max |rgb difference| {float((pr_img - ex_img).abs().max()):.3e}")


FIDELITY_K = 1.5         # measured d_prop / d_seed = 1.002 on an MI355X, x 1.5 (profiles/r19_proposal_render.md, "fidelity test")


def test_fidelity_against_the_exact_routes_own_spread():
    """d_prop = mean |proposal - exact| over the pixels of one seed against d_seed = mean |exact(seed a) - exact(seed b)|, the exact route's
    own Monte-Carlo spread from its jitter and u draws: tiny generator, 16 x 16, N = 12, relu, no noise, 33^3 lattice.  Asserted:
    d_prop <= FIDELITY_K * d_seed, FIDELITY_K = the ratio measured on an MI355X x 1.5 (profiles/r19_proposal_render.md, "fidelity test")."""
    gen, film, meta = _tiny_generator()
    S_, N = 16, 12
    kw = _kw(S_, N, nerf_noise=0.0)
    fg, pg, fa, pa = film["freq_geo"], film["phase_geo"], film["freq_app"], film["phase_app"]
    cube = callers.baked_cube_length(kw["fov"], kw["ray_start"], kw["ray_end"], num_steps=N)
    field = callers.bake_density(gen, None, film=meta, resolution=33, cube_length=cube)
    torch.manual_seed(5)
    exact_a = gen.staged_forward_with_frequencies(fg, fa, pg, pa, **kw)[0]
    torch.manual_seed(6)
    exact_b = gen.staged_forward_with_frequencies(fg, fa, pg, pa, **kw)[0]
    torch.manual_seed(5)
    prop = field.render(gen, **kw)[0]
    d_prop = float((prop - exact_a).abs().mean())
    d_seed = float((exact_b - exact_a).abs().mean())
    print(f"fidelity, 16x16, N = 12, 33^3 lattice: d_prop {d_prop:.4e}, d_seed {d_seed:.4e}, ratio {d_prop / d_seed:.3f}")
    assert d_seed > 0
    assert d_prop <= FIDELITY_K * d_seed
