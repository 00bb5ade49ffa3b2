"""fenerf_volume_sample / _sample_rays / _render (fenerf_amd/csrc/fenerf_volume.hip) against their numpy restatement
(fenerf_amd/volume_emulation.py, itself held to fp64 grid_sample by tests/test_volume_cpu.py) bit for bit, against the chain of public calls
the render stands for, against the field a lattice was baked from, and callers.bake_field / BakedField / render_multiview(baked=) end to end."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from test_gpu_parity import DEV, N_, T, _siren_module, proc
from test_gpu_pose_grads import _double_generator
from fenerf_amd import _lib, callers, native, volume_emulation as V
from fenerf_amd.generators import volumetric_rendering as VR

pytestmark = pytest.mark.gpu

OUT = -1e30


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _frame(shape):
    """a frame that is no power of two: the lattice spans [-0.18, 0.18] on every axis"""
    return (-0.18,) * 3, tuple(float(np.float32(0.36) / np.float32(n - 1)) for n in shape)


def _lattice(shape, ld, seed=0):
    return np.random.default_rng(seed).uniform(-1, 1, tuple(shape) + (ld,)).astype(np.float32)


def _point_pool(shape, origin, spacing, seed=1):
    """inside points, every node, both boundary planes of every axis (and their fp32 neighbours), outside points, NaN and +-inf"""
    rng = np.random.default_rng(seed)
    o, s, n = np.array(origin, np.float32), np.array(spacing, np.float32), np.array(shape)
    inside = (o + (rng.uniform(0, 1, (900, 3)) * (n - 1)).astype(np.float32) * s).astype(np.float32)
    idx = np.stack(np.meshgrid(*(np.arange(k) for k in shape), indexing="ij"), -1).reshape(-1, 3)
    nodes = (o + idx.astype(np.float32) * s).astype(np.float32)
    special = []
    for k in range(3):
        last = np.float32(o[k] + np.float32(shape[k] - 1) * s[k])
        for v in (o[k], np.nextafter(o[k], np.float32(-np.inf)), np.nextafter(o[k], np.float32(np.inf)), last, np.nextafter(last, np.float32(np.inf)),
                  np.nextafter(last, np.float32(-np.inf)), np.float32(o[k] - 0.05), np.float32(last + 0.05), np.nan, np.inf, -np.inf, np.float32(3e38)):
            for _ in range(3):
                p = inside[rng.integers(len(inside))].copy()
                p[k] = v
                special.append(p)
    pool = np.concatenate([inside, nodes, np.array(special, np.float32)])
    return pool[rng.permutation(len(pool))]


@pytest.mark.parametrize("C_,ld", [(1, 1), (3, 3), (22, 22), (22, 24)])      # ld % 4 != 0: the dword path; (22, 24): the 16-byte path
@pytest.mark.parametrize("shape", [(5, 4, 3), (8, 8, 8)])
def test_sampler_vs_emulation_bit_for_bit(shape, C_, ld):
    origin, spacing = _frame(shape)
    vol = _lattice(shape, ld)
    pool = _point_pool(shape, origin, spacing)
    assert len(pool) >= 1000
    dvol = T(vol)
    for P in (0, 1, 63, 64, 65, 1000):
        pts = pool[:P]
        got = native.volume_sample(dvol, origin, spacing, T(pts.reshape(P, 3)), OUT, C_)
        assert got.shape == (P, C_) and got.dtype == torch.float32 and got.is_cuda
        want = V.sample(vol, origin, spacing, pts, OUT, C_)
        differ = _bits(N_(got)) != _bits(want)
        assert not differ.any(), f"P = {P}: {int(differ.sum())} of {want.size} values differ in their bits"
    want = V.sample(vol, origin, spacing, pool[:1000], OUT, C_)
    n_out = int((want[:, -1] == np.float32(OUT)).sum())
    assert 20 < n_out < 500 and np.isfinite(want).all()                      # the mix holds inside and outside points
    if ld == 24:
        # the same lattice 4 bytes off a 16-byte boundary takes the dword path: the same bits
        flat = torch.empty(vol.size + 1, dtype=torch.float32, device=DEV)
        off = flat[1:].view(*vol.shape)
        off.copy_(dvol)
        assert off.data_ptr() % 16 == 4 and off.is_contiguous()
        got = native.volume_sample(off, origin, spacing, T(pool[:1000]), OUT, C_)
        assert np.array_equal(_bits(N_(got)), _bits(want))


def _rays(B, R, N, seed=3):
    """rays from around (0, 0, 0.45) through the lattice of _frame: the first and last samples of most rays are outside it"""
    rng = np.random.default_rng(seed)
    o = (np.array([0.0, 0.0, 0.45]) + rng.normal(0, 0.02, (B, R, 3))).astype(np.float32)
    d = np.array([0.0, 0.0, -1.0]) + rng.normal(0, 0.25, (B, R, 3))
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)
    z = np.sort(rng.uniform(0.2, 0.75, (B, R, N)), axis=-1).astype(np.float32)
    return o, d, z


@pytest.mark.parametrize("N", [3, 12])
def test_ray_form_vs_point_form_bit_for_bit(N):
    shape, B, R = (8, 8, 8), 2, 5
    origin, spacing = _frame(shape)
    vol = T(_lattice(shape, 24))
    o, d, z = (T(a) for a in _rays(B, R, N))
    assert (B * R * N) % 64 != 0
    p = o.unsqueeze(2) + d.unsqueeze(2) * z.unsqueeze(-1)              # torch, fp32, on the device: one multiply, one add
    by_point = native.volume_sample(vol, origin, spacing, p, OUT, 22)
    by_ray = native.volume_sample_rays(vol, origin, spacing, o, d, z, OUT, 22)
    assert by_ray.shape == (B, R, N, 22) and np.array_equal(_bits(N_(by_ray)), _bits(N_(by_point)))
    outside = N_(by_ray)[..., -1] == np.float32(OUT)
    assert outside.any() and (~outside).any()
    assert np.array_equal(_bits(N_(by_ray)), _bits(V.sample(N_(vol), origin, spacing, V.ray_points(N_(o), N_(d), N_(z)), OUT, 22).reshape(B, R, N, 22)))


def _render_case(seed=5):
    shape, B, R, N = (8, 8, 8), 2, 16, 12
    origin, spacing = _frame(shape)
    vol = _lattice(shape, 24, seed)
    vol[..., 21] *= 40.0                               # densities that make weights: about half of them negative (empty under relu)
    vol[..., 18:21] = vol[..., 18:21] * 0.5 + 0.5
    o, d, z = _rays(B, R, N, seed + 1)
    rng = np.random.default_rng(seed + 2)
    u = rng.uniform(0, 1, (B * R, N)).astype(np.float32)
    nc = rng.normal(size=(B, R, N)).astype(np.float32)
    nf = rng.normal(size=(B, R, 2 * N)).astype(np.float32)
    return shape, origin, spacing, T(vol), T(o), T(d), T(z), T(u), T(nc), T(nf)


OPTS = {"relu": dict(clamp_mode="relu"), "softplus_white": dict(clamp_mode="softplus", white_back=True), "relu_last": dict(clamp_mode="relu", last_back=True)}


@pytest.mark.parametrize("kind", sorted(OPTS))
def test_render_equals_the_chain_of_public_calls(kind):
    shape, origin, spacing, vol, o, d, z, u, nc, nf = _render_case()
    B, R, N = z.shape
    for hier in (True, False):
        for noise_std in (0.0, 0.7):
            opts = _lib.composite_opts(noise_std=noise_std, **OPTS[kind])
            copts = _lib.composite_opts(OPTS[kind]["clamp_mode"], noise_std)
            noise_c = nc if noise_std else None
            noise_f = (nf if hier else nf[..., :N].contiguous()) if noise_std else None
            got = native.volume_render(vol, origin, spacing, o, d, z, u if hier else None, noise_c if hier else None, noise_f, opts, OUT, 22,
                                       hierarchical=hier, want_weights=True, want_wsum=True)
            coarse = native.volume_sample_rays(vol, origin, spacing, o, d, z, OUT, 22)
            if hier:
                _, _, w, _ = native.composite(coarse, z, noise_c, copts)
                zf = native.resample(z.reshape(B * R, N), w.reshape(B * R, N), u)
                fine = native.volume_sample_rays(vol, origin, spacing, o, d, zf.reshape(B, R, N), OUT, 22)
                want = native.merge_composite(fine.reshape(B * R, N, 22), coarse.reshape(B * R, N, 22), zf, z.reshape(B * R, N), noise_f, opts)[:4]
            else:
                want = native.composite(coarse, z, noise_f, opts)
            for name, a, b in zip(("rgb", "depth", "weights", "wsum"), got, want):
                a, b = N_(a).reshape(-1), N_(b).reshape(-1)
                assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), (kind, hier, noise_std, name, float(np.abs(a - b).max()))
            rgb, wsum = N_(got[0]), N_(got[3])
            assert np.isfinite(rgb).all() and wsum.max() > 0.5                               # the rays meet matter


def _render_args(shape, origin, spacing, vol, o, d, z, u, nc, nf, hier=1):
    """the argument list of fenerf_volume_render for the case above, as a dict in declaration order"""
    B, R, N = z.shape
    M = 2 * N if hier else N
    nbytes = _lib.lib().fenerf_volume_render_workspace_bytes(B, R, N, 22, hier)
    keep = dict(ws=torch.empty(nbytes, dtype=torch.uint8, device=DEV), rgb=torch.empty((B, R, 21), device=DEV), depth=torch.empty((B, R), device=DEV),
                w=torch.empty((B, R, M), device=DEV), wsum=torch.empty((B, R), device=DEV), opts=_lib.composite_opts("relu", 0.5))
    p = lambda t: C.c_void_p(t.data_ptr())
    args = dict(vol=p(vol), n0=shape[0], n1=shape[1], n2=shape[2], C=22, ld=24, origin=(C.c_float * 3)(*origin), spacing=(C.c_float * 3)(*spacing),
                outside_last=OUT, B=B, R=R, N=N, hierarchical=hier, origins=p(o), dirs=p(d), z_coarse=p(z), u=p(u), noise_coarse=p(nc), noise_final=p(nf),
                opts=C.byref(keep["opts"]), out_rgb=p(keep["rgb"]), out_depth=p(keep["depth"]), out_weights=p(keep["w"]), out_wsum=p(keep["wsum"]),
                workspace=p(keep["ws"]), workspace_bytes=nbytes, stream=None)
    return args, keep


def test_render_and_sampler_refusals():
    """every refusal include/fenerf.h lists, one fault at a time: FENERF_E_INVALID with a message, before anything is launched"""
    case = _render_case()
    shape, origin, spacing, vol, o, d, z, u, nc, nf = case
    l = _lib.lib()
    good, keep = _render_args(*case)
    assert l.fenerf_volume_render(*good.values()) == _lib.OK
    torch.cuda.synchronize()
    f3 = lambda *v: (C.c_float * 3)(*v)
    faults = [(dict(vol=None), "NULL"), (dict(origin=None), "NULL"), (dict(spacing=None), "NULL"), (dict(origins=None), "NULL"), (dict(dirs=None), "NULL"),
              (dict(z_coarse=None), "NULL"), (dict(out_rgb=None), "NULL"), (dict(u=None), "needs u"), (dict(opts=None), "opts is NULL"),
              (dict(workspace=None), "workspace too small"), (dict(workspace_bytes=good["workspace_bytes"] - 1), "workspace too small"),
              (dict(n0=1), "at least 2 points"), (dict(n1=1), "at least 2 points"), (dict(n2=1), "at least 2 points"),
              (dict(C=0), "1 <= C <= 64"), (dict(C=65, ld=65), "1 <= C <= 64"), (dict(ld=21), "ld >= C"), (dict(C=1), "C >= 2"),
              (dict(spacing=f3(0.0, 0.1, 0.1)), "finite and positive"), (dict(spacing=f3(0.1, -0.1, 0.1)), "finite and positive"),
              (dict(spacing=f3(0.1, 0.1, float("inf"))), "finite and positive"), (dict(spacing=f3(float("nan"), 0.1, 0.1)), "finite and positive"),
              (dict(B=-1), "negative count"), (dict(R=-1), "negative count"), (dict(N=-1), "negative count"),
              (dict(N=2), "num_steps >= 3"), (dict(N=513), "samples per ray"), (dict(N=1025, hierarchical=0), "samples per ray"), (dict(N=0), "samples per ray")]
    for change, text in faults:
        rc = l.fenerf_volume_render(*dict(good, **change).values())
        msg = l.fenerf_last_error().decode()
        assert rc == _lib.E_INVALID and text in msg, (change, rc, msg)
    assert l.fenerf_volume_render(*dict(good, B=0).values()) == _lib.OK and l.fenerf_volume_render(*dict(good, R=0).values()) == _lib.OK
    # the sampler's two forms
    P = 7
    pts, rows, zs = torch.zeros((P, 3), device=DEV), torch.empty((P, 22), device=DEV), torch.zeros((P,), device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    lat = {k: good[k] for k in ("vol", "n0", "n1", "n2", "C", "ld", "origin", "spacing", "outside_last")}
    pgood = dict(lat, P=P, points=p(pts), rows=p(rows), stream=None)
    rgood = dict(lat, B=1, R=1, N=P, origins=p(pts), dirs=p(pts), z=p(zs), rows=p(rows), stream=None)
    assert l.fenerf_volume_sample(*pgood.values()) == _lib.OK and l.fenerf_volume_sample_rays(*rgood.values()) == _lib.OK
    shared = [(dict(vol=None), "NULL"), (dict(origin=None), "NULL"), (dict(spacing=None), "NULL"), (dict(rows=None), "NULL"), (dict(n1=1), "at least 2 points"),
              (dict(C=0), "1 <= C <= 64"), (dict(C=65, ld=65), "1 <= C <= 64"), (dict(ld=21), "ld >= C"), (dict(spacing=f3(0.1, 0.0, 0.1)), "finite and positive")]
    for fn, base, own in ((l.fenerf_volume_sample, pgood, [(dict(points=None), "NULL"), (dict(P=-1), "negative count")]),
                          (l.fenerf_volume_sample_rays, rgood, [(dict(origins=None), "NULL"), (dict(dirs=None), "NULL"), (dict(z=None), "NULL"),
                                                                (dict(B=-1), "negative count"), (dict(R=-1), "negative count"), (dict(N=-1), "negative count")])):
        for change, text in shared + own:
            rc = fn(*dict(base, **change).values())
            msg = l.fenerf_last_error().decode()
            assert rc == _lib.E_INVALID and text in msg, (fn.__name__, change, rc, msg)
    assert l.fenerf_volume_sample(*dict(pgood, P=0).values()) == _lib.OK and l.fenerf_volume_sample_rays(*dict(rgood, R=0).values()) == _lib.OK
    torch.cuda.synchronize()


RAW_FREQUENCY = -1.5         # 15 raw + 30 = 7.5


def test_the_lattice_is_the_field_convergence():
    """Trilinear interpolation is second order: a 4 x finer lattice of the same cube gives about 16 x less error once the lattice resolves the
    field; required here: err(33) <= err(9) / 4.  A swapped axis, a wrong origin or an off-by-one spacing does not converge.
    The field: the procedural baseline SIREN (no feature grid) at hidden width 32 with constant raw FiLM frequencies.  On the CPU
    (oracle/fenerf_oracle.py + volume_emulation.py, the same cube, the same 4,096 points) the reference alone gives, by raw frequency:
      -1.9 and -1.95 (effective 1.5, 0.75): err(9) = err(33) = 2e-7 -- the field is flat to fp32 rounding over the cube, nothing to converge;
      -1.7: 5.2e-6 -> 6.0e-7 (ratio 0.11);  -1.5: 1.9e-4 -> 1.2e-5 (0.061 = 1 / 16);  -1.2: 3.5e-3 -> 2.8e-4 (0.079);  -1.0: 0.14;  -0.5: 0.27.
    -1.5 is the one in the second-order regime with both errors well above rounding (and above the f16x3 kernel's own error)."""
    mod, spec, sd = _siren_module("baseline", 32, 0)
    gen = _double_generator(mod).eval()
    film = {k: T(np.full_like(v, RAW_FREQUENCY) if k.startswith("freq") else v) for k, v in proc.film_params(spec, 1, seed=4).items()}
    meta = dict(truncated_frequencies_geo=film["freq_geo"], truncated_phase_shifts_geo=film["phase_geo"],
                truncated_frequencies_app=film["freq_app"], truncated_phase_shifts_app=film["phase_app"])
    cube = callers.baked_cube_length(12, 0.88, 1.12, num_steps=6)
    q = T(np.random.default_rng(0).uniform(-cube / 2, cube / 2, (4096, 3)))
    with torch.no_grad():
        exact = N_(mod.native(torch.device(DEV)).siren_forward(q[None], None, film["freq_geo"], film["phase_geo"], film["freq_app"], film["phase_app"])[0])
    err = {}
    for n in (9, 33):
        field = callers.bake_field(gen, None, film=meta, resolution=n, cube_length=cube, max_points=n * n * 4)        # several slabs
        assert tuple(field.vol.shape) == (n, n, n, 24) and field.C == 22 and field.ld == 24
        got = N_(field.sample(q))
        assert got.shape == (4096, 22) and not (got[:, -1] == np.float32(callers.BAKED_OUTSIDE_SIGMA)).any()
        err[n] = float(np.abs(got - exact).max())
    print(f"baked lattice vs the exact SIREN at 4,096 points: err(9) {err[9]:.3e}, err(33) {err[33]:.3e}, ratio {err[33] / err[9]:.4f}")
    assert err[33] <= err[9] / 4


def _tiny_generator():
    torch.manual_seed(0)                  # the mapping networks of the module are torch-initialised
    mod, spec, sd = _siren_module("texture", 32, 6, sigma_gain=150.0)
    gen = _double_generator(mod).eval()
    film = {k: T(v) for k, v in proc.film_params(spec, 1, seed=4).items()}
    meta = dict(truncated_frequencies_geo=film["freq_geo"], truncated_phase_shifts_geo=film["phase_geo"],
                truncated_frequencies_app=film["freq_app"], truncated_phase_shifts_app=film["phase_app"])
    return gen, film, meta


def test_python_route_bake_render_multiview():
    gen, film, meta = _tiny_generator()
    S_, N = 8, 6
    kw = dict(img_size=S_, fov=12, ray_start=0.88, ray_end=1.12, num_steps=N, h_stddev=0.3, v_stddev=0.155, h_mean=math.pi / 2, v_mean=math.pi / 2,
              hierarchical_sample=True, sample_dist="gaussian", clamp_mode="relu", nerf_noise=0.1, last_back=False,
              fill_mode="eval_seg_padding_background", fill_color="black")
    cube = callers.baked_cube_length(kw["fov"], kw["ray_start"], kw["ray_end"], num_steps=N)
    field = callers.bake_field(gen, None, film=meta, resolution=17, cube_length=cube)
    assert tuple(field.vol.shape) == (17, 17, 17, 24) and field.vol.is_cuda and field.outside_last == -1e30
    # the lattice holds the SIREN's rows at origin + i * spacing
    i = torch.tensor([[0, 0, 0], [16, 16, 16], [3, 9, 14]], device=DEV)
    nodes = torch.tensor(field.origin, device=DEV) + i.float() * torch.tensor(field.spacing, device=DEV)
    pts = torch.cat([nodes, nodes[-1:].expand(29, -1)])[None].contiguous()
    rows = gen.siren.native(torch.device(DEV)).siren_forward(pts, None, film["freq_geo"], film["phase_geo"], film["freq_app"], film["phase_app"])[0, :3]
    assert np.array_equal(_bits(N_(field.vol[i[:, 0], i[:, 1], i[:, 2], :22])), _bits(N_(rows)))
    # layout, dtype and device of staged_forward_with_frequencies; one seed: the same rays, depths and noise
    torch.manual_seed(5)
    exact = gen.staged_forward_with_frequencies(film["freq_geo"], film["freq_app"], film["phase_geo"], film["phase_app"], lock_view_dependence=True, **kw)
    torch.manual_seed(5)
    baked = field.render(gen, **kw)
    assert len(baked) == len(exact) == 3
    for a, b in zip(baked, exact):
        assert a.shape == b.shape and a.dtype == b.dtype and a.device == b.device
    assert tuple(baked[0].shape) == (1, 22, S_, S_) and tuple(baked[1].shape) == (1, S_, S_)
    print(f"baked 17^3 vs exact locked-view render, {S_}x{S_}, {N}+{N} samples: max |pixel difference| {float((baked[0] - exact[0]).abs().max()):.3e} "
          f"(labels {float((baked[0][:, :19] - exact[0][:, :19]).abs().max()):.3e}, rgb {float((baked[0][:, 19:] - exact[0][:, 19:]).abs().max()):.3e})")
    # pixels bit for bit those of native.volume_render fed with the same draws
    R = S_ * S_
    rng = np.random.default_rng(9)
    rec = [rng.uniform(0, 1, (1, R, N, 1)), rng.normal(size=(1, 1)), rng.normal(size=(1, 1)), rng.normal(size=(1, R, N, 1)), rng.uniform(0, 1, (R, N)),
           rng.normal(size=(1, R, 2 * N, 1))]
    rec = [a.astype(np.float32) for a in rec]
    gen.draws = VR.RecordedDraws(rec)
    try:
        px, depth, _ = field.render(gen, **kw)
        assert not gen.draws.arrays, "all recorded draws consumed, in order"
    finally:
        del gen.draws
    o, d, z, _, _ = VR.sample_rays(1, N, DEV, kw["fov"], (S_, S_), kw["ray_start"], kw["ray_end"], kw["h_stddev"], kw["v_stddev"], kw["h_mean"], kw["v_mean"],
                                   kw["sample_dist"], draws=VR.RecordedDraws(rec[:3]))
    opts = _lib.composite_opts("relu", kw["nerf_noise"], False, False, False, kw["fill_mode"], kw["fill_color"])
    rgb, dep, _, _ = native.volume_render(field.vol, field.origin, field.spacing, o, d, z, T(rec[4]), T(rec[3]).reshape(1, R, N), T(rec[5]).reshape(1, R, 2 * N),
                                          opts, field.outside_last, field.C, hierarchical=True)
    want = gen._finish_scaled(rgb, 1, S_)
    assert np.array_equal(_bits(N_(px)), _bits(N_(want))) and np.array_equal(_bits(N_(depth)), _bits(N_(dep.reshape(1, S_, S_))))
    # no-grad only
    g_meta = dict(meta, truncated_frequencies_geo=film["freq_geo"].clone().requires_grad_(True))
    with pytest.raises(RuntimeError):
        callers.bake_field(gen, None, film=g_meta, resolution=5, cube_length=cube)
    g_field = callers.BakedField(field.vol, field.origin, field.spacing, field.C, (g_meta["truncated_frequencies_geo"],) + tuple(field.film[1:]))
    with pytest.raises(RuntimeError):
        g_field.render(gen, **kw)
    # render_multiview(baked=17): the shapes of the exact call
    cur = {0: dict(num_steps=3, img_size=S_), "fov": 12, "ray_start": 0.88, "ray_end": 1.12, "h_stddev": 0.3, "v_stddev": 0.155, "h_mean": math.pi / 2,
           "v_mean": math.pi / 2, "sample_dist": "gaussian", "clamp_mode": "relu", "hierarchical_sample": True, "fill_mode": "eval_seg_padding_background"}
    angles = (-0.3, 0.0, 0.3)
    ex_img, ex_seg = callers.render_multiview(gen, cur, 1, DEV, face_angles=angles, image_size=S_, lock_view_dependence=True, z_dim=8)
    bk_img, bk_seg = callers.render_multiview(gen, cur, 1, DEV, face_angles=angles, image_size=S_, lock_view_dependence=True, z_dim=8, baked=17)
    assert bk_img.shape == ex_img.shape == (3, 3, S_, S_) and bk_seg.shape == ex_seg.shape and bk_img.dtype == ex_img.dtype and bk_seg.dtype == ex_seg.dtype
    assert torch.isfinite(bk_img).all()
    print(f"render_multiview baked=17 vs exact, 3 views: max |rgb difference| {float((bk_img - ex_img).abs().max()):.3e}")
