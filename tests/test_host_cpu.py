"""CPU tests of the host-side logic (no GPU, no HIP compute): curriculum data, ray/camera sampling in torch vs the
golden vectors captured from the reference, draw order, error behaviour of the API surface."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, load_golden
from fenerf_amd import curriculums, _lib
from fenerf_amd.generators import generators as G
from fenerf_amd.generators import volumetric_rendering as VR
from fenerf_amd import procedural as proc
from fenerf_amd.siren import siren as S


def test_curriculums_match_reference_values():
    ref = json.load(open(os.path.join(GOLDEN, "curriculums.json")))
    for name, d in ref.items():
        mine = getattr(curriculums, name)
        got = {(f"int:{k}" if isinstance(k, int) else k): (list(v) if isinstance(v, tuple) else v) for k, v in mine.items()}
        assert got == d, name
    md = curriculums.extract_metadata(curriculums.CelebA_double_semantic_texture_embedding_256_dim_96, 60000)
    assert md["img_size"] == 128 and md["num_steps"] == 24 and md["model"].endswith("DIM_96")
    assert curriculums.next_upsample_step(curriculums.CelebA_double_semantic_texture_embedding_256_dim_96, 0) == 20000
    assert curriculums.last_upsample_step(curriculums.CelebA_double_semantic_texture_embedding_256_dim_96, 30000) == 20000


def test_rays_camera_host_functions():
    g = load_golden("camera_rays")
    for j in range(3):
        S_, N = int(g[f"r{j}_S"]), int(g[f"r{j}_N"])
        p, z, d = VR.get_initial_rays_trig(2, N, "cpu", 12, (S_, S_), 0.88, 1.12)
        np.testing.assert_allclose(p.numpy(), g[f"r{j}_points"], atol=1e-7)
        np.testing.assert_allclose(z.numpy(), g[f"r{j}_z"], atol=1e-7)
        np.testing.assert_allclose(d.numpy(), g[f"r{j}_dirs"], atol=1e-7)
    for i in range(int(g["n_modes"])):
        mode = str(g[f"m{i}_mode"])
        draws = VR.RecordedDraws(list(g[f"m{i}_draws"]))
        o, phi, theta = VR.sample_camera_positions("cpu", n=6, r=1, horizontal_stddev=0.3, vertical_stddev=0.155,
                                                   horizontal_mean=np.pi * 0.5, vertical_mean=np.pi * 0.5, mode=mode, draws=draws)
        assert not draws.arrays
        np.testing.assert_allclose(o.numpy(), g[f"m{i}_origin"], atol=1e-7)
        np.testing.assert_allclose(phi.numpy(), g[f"m{i}_phi"], atol=1e-7)
        c2w = VR.create_cam2world_matrix(VR.normalize_vecs(-o), o, device="cpu")
        np.testing.assert_allclose(c2w.numpy(), g[f"m{i}_cam2world"], atol=1e-7)
    # 'hybrid' (both branches of the coin) and 'truncated_gaussian', teacher-forced through `draws` like every other mode
    seen = set()
    for k in range(int(g["n_extra_modes"])):
        mode = str(g[f"x{k}_mode"])
        recorded = [g[f"x{k}_draw{j}"] for j in range(int(g[f"x{k}_n_draws"]))]
        draws = VR.RecordedDraws(recorded)
        o, phi, theta = VR.sample_camera_positions("cpu", n=5, r=1, horizontal_stddev=0.3, vertical_stddev=0.155,
                                                   horizontal_mean=np.pi * 0.5, vertical_mean=np.pi * 0.5, mode=mode, draws=draws)
        assert not draws.arrays, "every recorded draw consumed, in order"
        np.testing.assert_allclose(o.numpy(), g[f"x{k}_origin"], atol=1e-7)
        np.testing.assert_allclose(phi.numpy(), g[f"x{k}_phi"], atol=1e-7)
        np.testing.assert_allclose(theta.numpy(), g[f"x{k}_theta"], atol=1e-7)
        seen.add((mode, bool(recorded[0] < 0.5)) if mode == "hybrid" else (mode, None))
    assert {("hybrid", True), ("hybrid", False), ("truncated_gaussian", None)} <= seen


def test_default_draws_consume_the_generators_like_the_reference_modes():
    """hybrid / truncated_gaussian with the default (non-recorded) draws: same torch + python RNG consumption as the reference's
    statements (:170-177, :195-205), i.e. a seeded run gives what the recorded-draw replay of the same seeds gives."""
    import random
    for mode in ("hybrid", "truncated_gaussian"):
        random.seed(3); torch.manual_seed(7)
        o1, p1, t1 = VR.sample_camera_positions("cpu", n=4, horizontal_stddev=0.3, vertical_stddev=0.155, mode=mode)
        random.seed(3); torch.manual_seed(7)
        if mode == "hybrid":
            coin = random.random()
            a, b = (torch.rand((4, 1)), torch.rand((4, 1))) if coin < 0.5 else (torch.randn((4, 1)), torch.randn((4, 1)))
            rec = [np.float64(coin), a.numpy(), b.numpy()]
        else:
            rec = [torch.empty((4, 1, 4)).normal_().numpy(), torch.empty((4, 1, 4)).normal_().numpy()]
        o2, p2, t2 = VR.sample_camera_positions("cpu", n=4, horizontal_stddev=0.3, vertical_stddev=0.155, mode=mode, draws=VR.RecordedDraws(rec))
        assert torch.equal(o1, o2) and torch.equal(p1, p2) and torch.equal(t1, t2)


@pytest.mark.parametrize("name", ["tiny_texture_fwd", "tiny_texture_fwd_nohier"])
def test_sample_rays_matches_reference_transform(name):
    """The lean ray setup the fused renderer uses == reference get_initial_rays_trig + transform_sampled_points."""
    g = load_golden(name)
    B, S_, N = int(g["meta_B"]), int(g["meta_S"]), int(g["meta_N"])
    draws = VR.RecordedDraws([g["rand_u_jitter"], g["rand_r_theta"], g["rand_r_phi"]])
    o, d, z, pitch, yaw = VR.sample_rays(B, N, "cpu", 12, (S_, S_), 0.88, 1.12, 0.3, 0.155, np.pi * 0.5, np.pi * 0.5, "gaussian", draws=draws)
    np.testing.assert_allclose(o.numpy(), g["st_origins"], atol=2e-7)
    np.testing.assert_allclose(d.numpy(), g["st_dirs"], atol=2e-7)
    np.testing.assert_allclose(z.numpy(), g["st_z_coarse"][..., 0], atol=2e-7)
    np.testing.assert_allclose(torch.cat([pitch, yaw], -1).numpy(), g["poses"], atol=1e-7)
    # points = o + d*z reproduces the reference's transformed points up to fp32 rounding
    pts = o[:, :, None, :] + d[:, :, None, :] * z[..., None]
    np.testing.assert_allclose(pts.numpy(), g["st_points"], atol=5e-7)
    # and the full reference-shaped API too
    draws = VR.RecordedDraws([g["rand_u_jitter"], g["rand_r_theta"], g["rand_r_phi"]])
    pc, zc, dc = VR.get_initial_rays_trig(B, N, "cpu", 12, (S_, S_), 0.88, 1.12)
    tp, tz, td, to, pi_, ya = VR.transform_sampled_points(pc, zc, dc, "cpu", h_stddev=0.3, v_stddev=0.155, h_mean=np.pi * 0.5,
                                                         v_mean=np.pi * 0.5, mode="gaussian", draws=draws)
    np.testing.assert_allclose(tp.numpy(), g["st_points"], atol=3e-7)
    np.testing.assert_allclose(tz.numpy(), g["st_z_coarse"], atol=1e-7)


def test_generator_surface_and_loud_failures():
    gen = G.DoubleImplicitGenerator3d(functools.partial(S.TextureEmbeddingPiGAN128SEMANTICDISENTANGLE, hidden_dim=32), 16, 16, 22)
    assert gen.channel_dim == 21 and gen.step == 0 and gen.epoch == 0 and hasattr(gen.siren, "geo_mapping_network")
    names = set(dict(gen.siren.named_parameters()))
    for k in ("network.0.layer.weight", "final_layer.bias", "color_layer_sine.2.layer.weight", "color_layer_linear.0.weight",
              "label_layer_linear.2.bias", "geo_mapping_network.network.8.weight", "spatial_embeddings"):
        assert k in names, k
    assert tuple(gen.siren.color_layer_sine[0].layer.weight.shape) == (32, 32 + 32 + 3)
    md = curriculums.extract_metadata(curriculums.CelebA_double_semantic_texture_embedding_256_dim_96, 0)
    with torch.no_grad(), pytest.raises(KeyError):       # callers add nerf_noise (train...py:277); reference KeyErrors too
        gen.device = torch.device("cpu")
        gen(torch.randn(1, 16), torch.randn(1, 16), **md)
    md["nerf_noise"] = 0.0
    gen.device = torch.device("cpu")
    gen.siren.device = gen.device
    z = torch.randn(1, 16)
    with pytest.raises(RuntimeError):              # grad mode takes the differentiable HIP path: no CPU path there either
        gen(z, z, **md)
    with torch.no_grad(), pytest.raises(RuntimeError):   # CPU device: there is no CPU render path
        gen(z, z, **md)
    with torch.no_grad(), pytest.raises(TypeError):      # reference: raise "Need to choose clamp mode" -> TypeError
        gen(z, z, **dict(md, clamp_mode=None))
    sg = G.ImplicitGenerator3d(functools.partial(S.SPATIALSIRENBASELINE, hidden_dim=32), 16, 4)
    f, p = sg.siren.mapping_network(torch.randn(2, 16))
    assert f.shape == (2, 9 * 32)
    fg, pg, fa, pa = sg.siren.split_film(f, p)
    assert fg.shape == (2, 8 * 32) and fa.shape == (2, 32) and torch.equal(fa, f[:, -32:])


def test_draw_order_matches_reference():
    """A.6: forward draws rand[B,R,N,1], randn[B,1] x2, randn[B,R,N,1], rand[B*R,N], randn[B,R,2N,1]."""
    log = []

    class Spy:
        def rand(self, shape, device):
            log.append(("rand", tuple(shape)))
            return torch.rand(shape)

        def randn(self, shape, device):
            log.append(("randn", tuple(shape)))
            return torch.randn(shape)

    gen = G.DoubleImplicitGenerator3d(functools.partial(S.SIRENBASELINESEMANTICDISENTANGLE, hidden_dim=32), 8, 8, 22)
    gen.draws = Spy()
    gen.device = torch.device("cpu")
    gen.siren.device = gen.device
    md = dict(img_size=4, fov=12, ray_start=0.88, ray_end=1.12, num_steps=5, h_stddev=0.3, v_stddev=0.155, h_mean=1.57, v_mean=1.57,
              hierarchical_sample=True, sample_dist="gaussian", clamp_mode="relu", nerf_noise=0.0)
    z = torch.randn(3, 8)
    with torch.no_grad(), pytest.raises(RuntimeError):
        gen(z, z, **md)   # stops at the GPU call, after every draw has been made
    assert log == [("rand", (3, 16, 5, 1)), ("randn", (3, 1)), ("randn", (3, 1)), ("randn", (3, 16, 5, 1)), ("rand", (48, 5)),
                   ("randn", (3, 16, 10, 1))]
    log.clear()
    with pytest.raises(RuntimeError):
        gen.staged_forward(z, z, **md)
    assert log[:2] == [("randn", (10000, 8)), ("randn", (10000, 8))] and log[2] == ("rand", (3, 16, 5, 1))


def test_composite_opts_mapping():
    o = _lib.composite_opts("softplus", 0.5, last_back=True, fill_mode="seg_padding_background", fill_color="light_grey")
    assert (o.clamp_mode, o.last_back, o.fill_mode, o.fill_enabled) == (2, 1, 2, 1) and abs(o.fill_value - 0.81) < 1e-7
    o = _lib.composite_opts("relu", fill_mode="eval_seg_padding_background", fill_color="none")
    assert o.fill_enabled == 0 and o.fill_mode == 3
    o = _lib.composite_opts("relu", fill_mode="something_else")
    assert o.fill_mode == 0


def test_mask2color_and_voxel_samples_match_reference():
    from fenerf_amd import callers
    g = load_golden("caller_helpers")
    np.testing.assert_array_equal(np.array([callers.COLOR_MAP[k] for k in range(19)], np.float32), g["color_map"])
    np.testing.assert_array_equal(callers.mask2color(torch.from_numpy(g["masks"])).numpy(), g["colors"])   # exact argmax semantics
    for N in (4, 5):
        s, vo, vs = callers.create_samples(N, [0, 0, 0], 0.3)
        np.testing.assert_array_equal(s.numpy(), g[f"samples_{N}"])
        assert abs(vs - float(g[f"voxel_size_{N}"])) < 1e-15
    kw = callers.multiview_kwargs(curriculums.CelebA_double_semantic_texture_embedding_256_dim_96, image_size=64)
    assert kw["num_steps"] == 48 and kw["img_size"] == 64 and kw["psi"] == 0.7 and kw["h_stddev"] == 0 and kw["nerf_noise"] == 0
    assert all(isinstance(k, str) for k in kw) and kw["fill_mode"] == "seg_padding_background"


def test_inversion_host_pieces_match_the_reference_script():
    """callers.mask2labels / mIOU / inversion_trajectory against the functions of inverse_render_double_semantic.py itself (:82-92,
    :122-126, :504-570; tests/golden/inversion_helpers.npz: AST-extracted from the reference source and executed by tools/make_golden.py)."""
    from fenerf_amd import callers
    g = load_golden("inversion_helpers")
    np.testing.assert_array_equal(callers.mask2labels(g["mask"], 18), g["labels_18"])
    np.testing.assert_array_equal(callers.mask2labels(g["mask"], 19), g["labels_19"])
    np.testing.assert_array_equal(callers.mIOU(torch.from_numpy(g["miou_source"]), torch.from_numpy(g["miou_target"])).numpy(), g["miou"])
    n = int(g["trajectory_num_frames"])
    for name in g["trajectory_names"]:
        mine = np.array(callers.inversion_trajectory(str(name), n, 12), dtype=np.float64)
        np.testing.assert_array_equal(mine, g["trajectory_" + str(name)], err_msg=str(name))
    assert g["trajectory_zoom"].shape == (50, 4)          # the script's zoom ignores --num_frames


def test_reference_checkpoint_unpickles_into_this_package():
    """generator.pth of the reference is a pickled nn.Module (train_double_latent_semantic.py:526) whose class paths are
    generators.generators.* / siren.siren.*; with the import aliases it loads as this package's drop-in classes."""
    import subprocess
    import sys
    code = (
        "import sys, torch; sys.path.insert(0, %r)\n"
        "from fenerf_amd import compat; compat.install_aliases()\n"
        "g = torch.load(%r, weights_only=False)\n"
        "assert type(g).__module__ == 'fenerf_amd.generators.generators' and type(g.siren).__module__ == 'fenerf_amd.siren.siren'\n"
        "assert g.siren.hidden_dim == 32 and g.output_dim == 22 and g.step == 0 and g.siren.gridwarper.scale_factor == 2 / 0.24\n"
        "import numpy as np; from fenerf_amd import procedural as proc\n"
        "spec = proc.model_spec('texture', hidden_dim=32, grid_size=8, z_dim=16)\n"
        "sd = proc.make_state_dict(spec, seed=3, sigma_gain=300.0)\n"
        "mine = g.siren.state_dict()\n"
        "assert set(mine) == set(sd) and all(np.array_equal(mine[k].numpy(), sd[k]) for k in sd)\n"
        "print('ok')\n") % (os.path.dirname(GOLDEN.rstrip('/')).rsplit('/tests', 1)[0], os.path.join(GOLDEN, "ref_generator_tiny.pth"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]


def test_reference_style_generator_unpickles_into_this_package():
    """A pickled StyleGenerator3d (generators.py:914; tests/golden/ref_style_generator_tiny.pth is the reference's own object) loads
    as fenerf_amd's class of that name -- round 4's review: 'a pickled one would not load'."""
    import subprocess
    import sys
    code = (
        "import sys, torch; sys.path.insert(0, %r)\n"
        "from fenerf_amd import compat; compat.install_aliases()\n"
        "g = torch.load(%r, weights_only=False)\n"
        "assert type(g).__name__ == 'StyleGenerator3d' and type(g).__module__ == 'fenerf_amd.generators.generators'\n"
        "assert type(g.siren).__name__ == 'SPATIALSIRENBASELINE' and g.z_dim == 16 and g.output_dim == 4 and not hasattr(g, 'avg_frequencies')\n"
        "import numpy as np; from fenerf_amd import procedural as proc\n"
        "sd = proc.make_state_dict(proc.model_spec('spatial', hidden_dim=32, z_dim=16), seed=8, sigma_gain=300.0)\n"
        "mine = g.siren.state_dict()\n"
        "assert set(mine) == set(sd) and all(np.array_equal(mine[k].numpy(), sd[k]) for k in sd)\n"
        "print('ok')\n") % (os.path.dirname(GOLDEN.rstrip('/')).rsplit('/tests', 1)[0], os.path.join(GOLDEN, "ref_style_generator_tiny.pth"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]


def test_ema_shim_matches_the_reference_usage(tmp_path):
    """train_double_latent_semantic.py:145,456,487-488 / render_multiview_images_double_semantic.py:62-64: an EMA object is
    pickled whole (torch.save(ema)) under the module path torch_ema.ema and later unpickled and copied into the generator."""
    import subprocess
    import sys
    import textwrap
    import torch
    from fenerf_amd import ema as E
    lin = torch.nn.Linear(3, 2)
    avg = E.ExponentialMovingAverage(lin.parameters(), decay=0.999)
    w0 = lin.weight.detach().clone()
    with torch.no_grad():
        lin.weight.add_(1.0)
    avg.update(lin.parameters())
    d = min(0.999, (1 + 1) / (10 + 1))                      # warm-up decay of the first update
    assert torch.allclose(avg.shadow_params[0], w0 + (1 - d) * 1.0)
    avg.store(lin.parameters()); avg.copy_to(lin.parameters())
    assert torch.equal(lin.weight.detach(), avg.shadow_params[0])
    avg.restore(lin.parameters())
    assert torch.allclose(lin.weight.detach(), w0 + 1.0)
    # a pickle that names torch_ema.ema.ExponentialMovingAverage, as the reference's *_ema.pth files do
    code = textwrap.dedent(f"""
        import sys, types, torch
        sys.path.insert(0, {repr(str(__import__('pathlib').Path(__file__).resolve().parents[1]))})
        from fenerf_amd import compat
        compat.install_aliases()
        import torch_ema
        e = torch_ema.ExponentialMovingAverage(torch.nn.Linear(3, 2).parameters(), decay=0.9)
        assert type(e).__module__ in ("fenerf_amd.ema", "torch_ema.ema")
        type(e).__module__ = "torch_ema.ema"
        torch.save(e, r"{tmp_path}/ema.pth")
        type(e).__module__ = "fenerf_amd.ema"
        back = torch.load(r"{tmp_path}/ema.pth", weights_only=False)
        lin = torch.nn.Linear(3, 2)
        back.copy_to(lin.parameters())
        assert torch.equal(lin.weight.detach(), e.shadow_params[0]) and back.decay == 0.9
        print("ok")
    """)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]


def _spatial_grid_module(g):
    H = int(g["meta_H"])
    mod = S.SPATIALSIRENGRID(input_dim=3, z_dim=16, hidden_dim=H, output_dim=4)
    sd = {k[2:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("w_")}
    gshapes = {n: tuple(p.shape) for n, p in mod.grid_latent_network.named_parameters()}
    sd.update({"grid_latent_network." + n: torch.from_numpy(v) for n, v in proc.latent_grid_state(gshapes, seed=31).items()})
    sd.update({k: v for k, v in mod.state_dict().items() if k.endswith("blur.kernel") or k.endswith("upsample.kernel")})   # buffers
    mod.load_state_dict(sd, strict=True)
    return mod


def test_spatial_siren_grid_host_pieces_match_the_reference():
    """fenerf_amd.siren.siren.SPATIALSIRENGRID: state dict identical in names and shapes to the reference module's (the StyleGAN2-style
    latent-grid generator included), its StyleGenerator2D reproduces the reference's latent grid from z, and the torch-side steps of
    forward() -- local-latent sampling, per-point mapping network, local coordinates -- reproduce the reference's stage outputs."""
    import json
    g = load_golden("tiny_spatial_grid")
    mod = _spatial_grid_module(g)
    ref_sd = json.loads(str(g["meta_state_dict"]))
    assert {k: list(v.shape) for k, v in mod.state_dict().items()} == ref_sd        # load_state_dict(reference, strict=True) compatible
    np.testing.assert_array_equal(mod.grid_latent_network.convs[0].blur.kernel.numpy(), g["blur_kernel"])
    with torch.no_grad():
        lat = mod.grid_latent_network(torch.from_numpy(g["z"]))
    err = np.abs(lat.numpy() - g["latent_grid"]).max() / np.abs(g["latent_grid"]).max()
    print(f"StyleGenerator2D vs the reference's latent grid: relative max error {err:.2e}")
    assert lat.shape == (2, 32, 32, 32) and err <= 1e-5
    pts = torch.from_numpy(g["points"])
    sampled = mod.sample_local_latents(torch.from_numpy(g["latent_grid"]), mod.gridwarper(pts))
    np.testing.assert_allclose(sampled.numpy(), g["sampled_latent"], atol=1e-6)
    with torch.no_grad():
        f, p = mod.mapping_network(sampled)
    np.testing.assert_allclose(f.numpy(), g["freq"], atol=2e-6)
    np.testing.assert_allclose(p.numpy(), g["phase"], atol=2e-6)
    np.testing.assert_allclose(mod.get_local_coordinates(pts, 32, preserve_y=False).numpy(), g["local_coords"], atol=1e-7)
    keep_y = mod.get_local_coordinates(pts, 32, preserve_y=True).numpy()
    np.testing.assert_array_equal(keep_y[..., 1], g["points"][..., 1])
    with pytest.raises(RuntimeError, match="GPU only"):          # the render itself has no CPU path
        with torch.no_grad():
            mod(pts, torch.from_numpy(g["z"]), torch.from_numpy(g["dirs"]))
    assert mod._spec()["n_color"] == 1 and mod._spec()["n_geo"] == 8
    assert not any(n.startswith("grid_latent_network") or "mapping_network" in n for n, _ in mod._named_render_params())


def test_style_generator_2d_variants_and_latent_formats():
    """skip_conn on / off, per-layer latent lists and [B, n_layers, z] latents (latent_grid.py:95-137), against the same algebra spelled
    with per-sample weights and a grouped convolution (the reference's formulation of modulated convolution)."""
    from fenerf_amd.siren import latent_grid as LG
    torch.manual_seed(0)
    for skip in (False, True):
        gen = LG.StyleGenerator2D(out_res=16, out_ch=5, z_dim=8, ch_mul=1, ch_max=16, skip_conn=skip).eval()
        z = torch.randn(3, 8)
        with torch.no_grad():
            a = gen(z)
            b = gen(gen.process_latents(z))                         # the list form passes through
            c = gen(z[:, None, :].expand(-1, gen.n_layers, -1))     # per-layer latents (normalised after the mapping network)
        assert a.shape == (3, 5, 16, 16) and torch.equal(a, b) and c.shape == a.shape
        assert gen.n_layers == len(gen.convs) + 2 + (len(gen.to_rgbs) if skip else 0)
    conv = LG.ModulatedConv2d(6, 4, 3, 8, upsample=True).eval()
    x, z = torch.randn(2, 6, 5, 5), torch.randn(2, 8)
    with torch.no_grad():
        got = conv(x, z)
        gamma = conv.modulation(z).view(2, 1, 6, 1, 1)
        w = conv.scale * conv.weight * gamma
        w = w * torch.rsqrt(w.pow(2).sum([2, 3, 4]) + 1e-8).view(2, 4, 1, 1, 1)
        wt = w.transpose(1, 2).reshape(12, 4, 3, 3)
        ref = torch.nn.functional.conv_transpose2d(x.view(1, 12, 5, 5), wt, stride=2, groups=2).view(2, 4, 11, 11)
        ref = conv.activate(conv.blur(ref))
    assert got.shape == (2, 4, 10, 10)
    np.testing.assert_allclose(got.numpy(), ref.numpy(), atol=2e-6)


def test_avg_frequency_cache_keeps_values_and_rng_consumption():
    """generate_avg_frequencies (generators.py:530-543, re-done by every staged_forward) is cached on (mapping weights, generator
    state before the draws): a re-seeded call returns bit-identical means AND leaves the generator where the two 10000-latent draws
    would have; another seed or changed weights recompute."""
    import functools
    import io
    gen = G.DoubleImplicitGenerator3d(functools.partial(S.SIRENBASELINESEMANTICDISENTANGLE, hidden_dim=32), 8, 8, 22)
    gen.device = torch.device("cpu"); gen.siren.device = gen.device
    calls = []
    orig = gen.siren.geo_mapping_network.forward
    gen.siren.geo_mapping_network.forward = lambda z: (calls.append(1), orig(z))[1]
    torch.manual_seed(3); a = [t.clone() for t in gen.generate_avg_frequencies()]; ra = torch.rand(3)
    torch.manual_seed(3); b = [t.clone() for t in gen.generate_avg_frequencies()]; rb = torch.rand(3)
    assert len(calls) == 1 and all(torch.equal(x, y) for x, y in zip(a, b)) and torch.equal(ra, rb)
    torch.manual_seed(4); c = [t.clone() for t in gen.generate_avg_frequencies()]
    assert len(calls) == 2 and not torch.equal(c[0], a[0])
    with torch.no_grad():
        next(gen.siren.geo_mapping_network.parameters()).add_(0.1)
    torch.manual_seed(4); d = gen.generate_avg_frequencies()
    assert len(calls) == 3 and not torch.equal(d[0], c[0])
    # writes through param.data (torch_ema's copy_to / restore) bypass the version counters: the same seed would hit the cache
    # with the OLD weights' averages -- the generator's eval() / train() (the reference brackets every EMA swap with them) and
    # invalidate_native() drop the cache
    w0 = next(gen.siren.geo_mapping_network.parameters())
    for how in ("eval", "train", "invalidate_native"):
        before = len(calls)
        torch.manual_seed(4); e0 = [t.clone() for t in gen.generate_avg_frequencies()]
        w0.data.copy_(w0.data * 1.5 + 0.01)
        getattr(gen, how)()
        torch.manual_seed(4); e1 = gen.generate_avg_frequencies()
        assert len(calls) - before >= 1 and not torch.equal(e1[0], e0[0]), how
    calls.clear(); calls.extend([1] * 3)
    gen.draws = VR.RecordedDraws([np.zeros((10000, 8), np.float32)] * 2)          # recorded draws are replayed, never cached
    gen.generate_avg_frequencies()
    assert len(calls) == 4 and not gen.draws.arrays
    gen.draws = VR._DEFAULT_DRAWS
    del gen.siren.geo_mapping_network.forward
    buf = io.BytesIO()
    torch.save(gen, buf)
    buf.seek(0)
    assert "_avg_cache" not in torch.load(buf, weights_only=False).__dict__


# ---------------------------------------------------------------------------------------------------
# the reference-side ctypes binding shown there is EXECUTED (round 4: the round-3 text built a description with
# abi_version=1 that the ABI-2 library rejects, and nothing noticed)
# ---------------------------------------------------------------------------------------------------
def integration_md_binding():
    """The ```python block of INTEGRATION.md that starts with '# reference: generators/fenerf_hip.py', executed as written against
    the in-tree library (FENERF_LIB).  -> its namespace"""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "INTEGRATION.md")).read()
    blocks = [b for b in re.findall(r"```python\n(.*?)```", text, flags=re.S) if b.startswith("# reference: generators/fenerf_hip.py")]
    assert len(blocks) == 1
    old = os.environ.get("FENERF_LIB")
    os.environ["FENERF_LIB"] = _lib.LIB_PATH
    try:
        ns = {}
        exec(compile(blocks[0], "INTEGRATION.md#B", "exec"), ns)
    finally:
        if old is None:
            del os.environ["FENERF_LIB"]
        else:
            os.environ["FENERF_LIB"] = old
    return ns


def _check_mirror(cls, struct_name):
    import ctypes as C
    l = _lib.lib()
    sname = struct_name.encode()
    assert C.sizeof(cls) == l.fenerf_struct_size(sname), struct_name
    names = []
    while l.fenerf_struct_field_name(sname, len(names)) is not None:
        names.append(l.fenerf_struct_field_name(sname, len(names)).decode())
    assert [f[0] for f in cls._fields_] == names, (struct_name, names)
    for n in names:
        assert getattr(cls, n).offset == l.fenerf_struct_field_offset(sname, n.encode()), (struct_name, n)


def test_integration_md_binding_structs_match_the_loaded_library():
    ns = integration_md_binding()
    assert ns["FENERF_ABI_VERSION"] == _lib.lib().fenerf_abi_version() == _lib.ABI_VERSION
    _check_mirror(ns["Desc"], "FenerfModelDesc")
    _check_mirror(ns["Opts"], "FenerfCompositeOpts")
    _check_mirror(ns["Grads"], "FenerfSirenGrads")
    # the package's own mirrors, all six structs of include/fenerf.h
    for cls, name in ((_lib.FenerfModelDesc, "FenerfModelDesc"), (_lib.FenerfCompositeOpts, "FenerfCompositeOpts"), (_lib.FenerfRepackMaps, "FenerfRepackMaps"),
                      (_lib.FenerfLocalMapDesc, "FenerfLocalMapDesc"), (_lib.FenerfSirenGrads, "FenerfSirenGrads"),
                      (_lib.FenerfMappingNet, "FenerfMappingNet")):
        _check_mirror(cls, name)
    l = _lib.lib()
    assert l.fenerf_struct_size(b"NoSuchStruct") == -1 and l.fenerf_struct_field_offset(b"FenerfModelDesc", b"nope") == -1
    assert l.fenerf_struct_field_name(b"FenerfModelDesc", 999) is None


@pytest.mark.parametrize("kind,precision", [("texture", 1), ("texture", 0), ("baseline", 1)])
def test_integration_md_binding_describes_the_model_the_package_packs(kind, precision):
    """desc_from_siren of the documented binding, on a module with the reference's attribute names, is accepted by the library
    (abi_version, field layout) and packs to exactly the stream the package's own binding packs from the same weights."""
    import ctypes as C
    ns = integration_md_binding()
    spec = proc.model_spec(kind, hidden_dim=32, grid_size=6, z_dim=8)
    sd = proc.make_state_dict(spec, seed=9, with_mapping=False)
    cls = {"texture": S.TextureEmbeddingPiGAN128SEMANTICDISENTANGLE, "baseline": S.SIRENBASELINESEMANTICDISENTANGLE}[kind]
    mod = cls(hidden_dim=32, z_geo_dim=8, z_app_dim=8, output_dim=22)
    tsd = {k: torch.from_numpy(v) for k, v in sd.items()}
    if "spatial_embeddings" in tsd:
        mod.spatial_embeddings = torch.nn.Parameter(tsd["spatial_embeddings"].clone())
    mod.load_state_dict(tsd, strict=False)
    d, keep = ns["desc_from_siren"](mod, precision=precision)
    assert (d.abi_version, d.hidden_dim, d.n_geo, d.n_color, d.n_label_layers, d.output_dim, d.grid_ch) == \
        (2, 32, 8, 3, spec["n_label_layers"], 22, spec["grid_ch"])
    l = ns["_l"]
    fp, sz = C.POINTER(C.c_float), C.c_size_t
    blob, consts, nb, nc = fp(), fp(), sz(), sz()
    rc = l.fenerf_pack_weights_host(C.byref(d), C.byref(blob), C.byref(nb), C.byref(consts), C.byref(nc))
    assert rc == 0, l.fenerf_last_error()
    try:
        got = np.ctypeslib.as_array(blob, shape=(nb.value,)).copy(), np.ctypeslib.as_array(consts, shape=(nc.value,)).copy()
    finally:
        l.fenerf_free_host.argtypes = [C.c_void_p]
        l.fenerf_free_host(blob)
        l.fenerf_free_host(consts)
    mine = _lib.pack_weights_host(sd, spec, "f16x3" if precision else "f32")
    assert np.array_equal(got[0], mine[0]) and np.array_equal(got[1], mine[1])
    # a stale ABI number -- the round-3 text -- is refused
    d.abi_version = 1
    assert l.fenerf_pack_weights_host(C.byref(d), C.byref(blob), C.byref(nb), C.byref(consts), C.byref(nc)) == _lib.E_INVALID
    assert b"abi_version" in l.fenerf_last_error()


def test_pickles_made_where_the_reference_cuda_ops_imported_still_load(tmp_path):
    """siren/op/__init__.py:1-4 of the reference imports FusedLeakyReLU from siren.op.fused_act when its CUDA extensions build, from
    siren.op.native_ops otherwise: a SPATIALSIRENGRID checkpoint pickled on the first kind of machine names the class under
    siren.op.fused_act.  compat.install_aliases() serves both paths (round-3 advisory)."""
    import subprocess
    import sys
    import textwrap
    code = textwrap.dedent(f"""
        import sys, torch
        sys.path.insert(0, {repr(str(__import__('pathlib').Path(__file__).resolve().parents[1]))})
        from fenerf_amd import compat
        compat.install_aliases()
        from fenerf_amd.siren import latent_grid as LG
        act = LG.FusedLeakyReLU(5)
        with torch.no_grad():
            act.bias.copy_(torch.arange(5.0))
        x = torch.randn(2, 5, 3, 3)
        for path in ("siren.op.fused_act", "siren.op.native_ops"):
            LG.FusedLeakyReLU.__module__ = path            # what the reference's pickle records on the two kinds of machine
            torch.save(act, r"{tmp_path}/act.pth")
            LG.FusedLeakyReLU.__module__ = "fenerf_amd.siren.latent_grid"
            back = torch.load(r"{tmp_path}/act.pth", weights_only=False)
            assert type(back) is LG.FusedLeakyReLU and torch.equal(back(x), act(x)), path
        import importlib
        assert importlib.import_module("siren.op.upfirdn2d") is LG
        print("ok")
    """)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]


def test_backward_chunk_plan_and_grid_digest():
    """Host logic of the differentiable path that needs no GPU: the chunk plan of the backward (whole images while they fit, point
    ranges of an image otherwise; every point exactly once) and the digest that lets a forced re-pack recognise an unchanged grid."""
    from fenerf_amd import native
    from fenerf_amd.siren import autograd as SA
    for nB, Pp, cap in ((12, 393216, 393216), (2, 393216, 196608), (8, 24576, 196608), (3, 544, 128), (4, 1700, 1700), (1, 786432, 1 << 30)):
        chunks = SA.plan_chunks(nB, Pp, cap)
        seen = np.zeros((nB, Pp), np.int32)
        for b, nb, s, n in chunks:
            limit = max(128, cap // 128 * 128)
            assert nb >= 1 and n >= 1 and (nb == 1 or (s == 0 and n == Pp)), "several images only as WHOLE images"
            assert nb * n <= limit or (nb == 1 and n <= limit), (nb, n, limit)
            seen[b:b + nb, s:s + n] += 1
        assert (seen == 1).all(), (nB, Pp, cap)
    assert SA.plan_chunks(12, 393216) == [(b, 1, 0, 393216) for b in range(12)] and SA.BACKWARD_CHUNK_POINTS == 393216 and SA.OVERLAP_WGRAD is False
    # digest: wrap-around int32 sums of runs of 1,024 words -- a single changed word changes it, and so does a pair of compensating edits
    # in DIFFERENT runs (which a single global sum would miss); equal content gives an equal digest
    g = torch.randn(1, 32, 8, 8, 8)
    d0 = native.NativeModel._grid_checksum(g)
    assert d0.shape == (16,) and d0.dtype == torch.int32 and torch.equal(d0, native.NativeModel._grid_checksum(g.clone()))
    h = g.clone().reshape(-1)
    bits = h.view(torch.int32)
    bits[5] += 7
    bits[5000] -= 7                      # same global sum, different runs
    assert int(bits.sum(dtype=torch.int32)) == int(g.reshape(-1).view(torch.int32).sum(dtype=torch.int32))
    assert not torch.equal(native.NativeModel._grid_checksum(h.reshape(g.shape)), d0)
    odd = torch.randn(1, 32, 3, 3, 5)    # 1,440 words: the run length falls back to a power of two that divides it (32)
    assert native.NativeModel._grid_checksum(odd).shape == (45,)


def test_backward_plan_of_the_c_abi_matches_the_python_planner_and_tiles_its_workspace():
    """backward_plan of fenerf_api.cpp -- the one object the render backward's workspace sizes, pointers and chunk loop come from --
    through its test hook, on the CPU: the chunk list is siren.autograd.plan_chunks' for the same arguments, and the regions start
    256-aligned, tile [0, total) in the declared order without gaps beyond the alignment, and are empty exactly where their rule says.
    The rows are those of test_backward_chunk_plan_and_grid_digest; the C entry plans 2 B (pass, image) pairs, so a row's nB is 2 B
    where it is even and B where it is odd.  A FiLM-only step of an f16x3 model plans by the FiLM-sums budget without ray gradients
    and by the dump's with them (the input-gradient pass reads the dump): there the ray modes are compared with each other only."""
    import ctypes as C
    from fenerf_amd.siren import autograd as SA
    hook = _lib.lib().fenerf_internal_backward_plan
    hook.restype = C.c_int
    hook.argtypes = [C.POINTER(C.c_int)] + [C.c_int] * 4 +[C.c_int64] * 2 + [C.c_int] * 2 + [C.POINTER(C.c_int64), C.c_int, C.POINTER(C.c_uint64)]
    names = ("d_out2", "d_fc", "dump", "d_grid_cl", "d_e", "det_ws", "wgrad", "film2", "scratch", "d_pts2", "d_rd2")
    H, ng, nc, ch, F16X3 = 64, 3, 2, 4, _lib.PRECISION["f16x3"]
    L = ng + nc
    chunks_buf, off_buf = (C.c_int64 * (4 * 256))(), (C.c_uint64 * 13)()

    def plan(prec, grid, det, B, R, N, film_only, chunk_points, budget, slots, ray):
        dims = (C.c_int * 13)(H, ng, nc, ch, 32 if grid else 0, *((8, 8, 8) if grid else (0, 0, 0)), prec, 1, int(det), 0, 256)
        n = hook(dims, B, R, N, film_only, chunk_points, budget, slots, ray, chunks_buf, 256, off_buf)
        assert 0 < n <= 256
        return [tuple(chunks_buf[4 * i:4 * i + 4]) for i in range(n)], list(off_buf)

    calls = 0
    for nB, Pp_row, cap in ((12, 393216, 393216), (2, 393216, 196608), (8, 24576, 196608), (3, 544, 128), (4, 1700, 1700), (1, 786432, 1 << 30)):
        B = nB // 2 if nB % 2 == 0 else nB
        R, N = (Pp_row // 4, 4) if Pp_row % 24 else (Pp_row // 24, 24)
        P, Pp = R * N, (R * N + 31) // 32 * 32
        assert P == Pp_row
        sums_bytes_pp = 4.0 * ((Pp + 127) // 128 * L * 2 * H) / Pp          # fenerf_siren_film_sums_floats(m, 1, Pp): one unit per 128 points
        budget = int(cap * sums_bytes_pp) + 64
        for prec, grid, det in ((p, g, d) for p in (_lib.PRECISION["f32"], F16X3) for g in (False, True) for d in ((False, True) if g else (False,))):
            for film_only in (0, 1):
                film16_possible = bool(film_only) and prec == F16X3
                for slots in (1, 2):
                    by_ray = {}
                    for ray in (0, 1, 2):
                        chunks, off = plan(prec, grid, det, B, R, N, film_only, cap, budget, slots, ray)
                        calls += 1
                        film16 = film16_possible and ray == 0
                        # (a) the chunk list
                        limit = int(min(float(1 << 24), budget / sums_bytes_pp)) if film16 else cap
                        assert chunks == SA.plan_chunks(2 * B, Pp, limit), (nB, Pp, cap, prec, film_only, ray)
                        # (b), (c) aligned, in order, disjoint, ending at total
                        starts, total, stride = off[:11], off[11], off[12]
                        assert all(s % 256 == 0 for s in starts) and total % 256 == 0 and stride % 256 == 0
                        assert starts[0] == 0 and all(a <= b for a, b in zip(starts, starts[1:] + [total]))
                        size = dict(zip(names, (b - a for a, b in zip(starts, starts[1:] + [total]))))
                        assert size["dump"] == stride * min(slots, len(chunks))
                        # (e) which regions are empty
                        det_on = grid and det and not film_only
                        scatters = prec == F16X3          # the f16x3 chain scatters d(grid features) itself
                        want = dict(d_out2=True, d_fc=Pp != P, dump=True, d_grid_cl=grid and not film_only and not det_on,
                                    d_e=det_on or (grid and not scatters), det_ws=det_on, wgrad=True, film2=True, scratch=len(chunks) > 1,
                                    d_pts2=ray != 0, d_rd2=ray == 1)
                        assert {k: v > 0 for k, v in size.items()} == {k: bool(v) for k, v in want.items()}, (size, want)
                        assert size["d_out2"] >= 2 * B * Pp * ch * 4 and size["film2"] >= 2 * B * 2 * L * H * 4
                        if ray:
                            assert size["d_pts2"] >= 2 * B * Pp * 3 * 4
                        by_ray[ray] = (chunks, starts[:10])
                    # (d) the ray regions lie behind everything else: nothing in front of them moves
                    assert by_ray[1] == by_ray[2]
                    if not film16_possible:
                        assert by_ray[0] == by_ray[1]
    assert calls == 6 * 6 * 2 * 2 * 3


def test_backward_gradient_sum_over_chunks_is_the_sequential_sum():
    """siren/autograd.py GradSum, the one sum of per-chunk gradients of the Python backward, over fake per-chunk results for plans from
    plan_chunks -- a plan is whole-image chunks (here 2 + 2 + 1 images) or point ranges of single images (here 4 x 128 + 32 points of
    each of 3 images), so both kinds are fed, and one sum is carried across both (the two-node backward hands its GradSum on):
    weight / bias gradients bit-identical to the left-to-right sum ((r0 + r1) + r2) ..., FiLM gradients one row per image in image
    order, each the left-to-right sum over that image's point ranges.  A result without a weight part (the FiLM-only route) sums too."""
    from fenerf_amd.siren import autograd as SA
    gen = torch.Generator().manual_seed(7)
    rnd = lambda *shape: torch.randn(*shape, generator=gen) * 10.0 ** torch.randint(-3, 4, shape, generator=gen).float()
    widths = dict(zip(SA.FILM_KEYS, (24, 24, 8, 8)))

    def fake(nb, weights=True):
        r = {k: rnd(nb, w) for k, w in widths.items()}
        if weights:
            r.update(geo_w=[rnd(8, 3), rnd(8, 8)], geo_b=[rnd(8), rnd(8)], head_w=rnd(32, 8), rgb_b=rnd(3))
        return r

    def check(plans, weights):
        chunks = [c for plan in plans for c in plan]
        results = [fake(nb, weights) for _, nb, _, _ in chunks]
        flat = lambda r: [t for k in sorted(r) if k not in SA.FILM_KEYS for t in (r[k] if isinstance(r[k], list) else [r[k]])]
        want_w = [t.clone() for t in flat(results[0])]
        for r in results[1:]:
            want_w = [a + b for a, b in zip(want_w, flat(r))]
        want_film = {k: [] for k in SA.FILM_KEYS}
        for (b, nb, s, n), r in zip(chunks, results):
            for k in SA.FILM_KEYS:
                if s == 0:
                    want_film[k].append(r[k].clone())
                else:
                    want_film[k][-1] = want_film[k][-1] + r[k]
        acc = SA.GradSum()
        for c, r in zip(chunks, results):
            acc.add(c, r)
        got = acc.result()
        assert sorted(got) == sorted(results[0])
        assert len(flat(got)) == len(want_w) and all(torch.equal(a, b) for a, b in zip(flat(got), want_w))
        images = sum(nb for _, nb, s, _ in chunks if s == 0)
        for k in SA.FILM_KEYS:
            assert got[k].shape == (images, widths[k]) and torch.equal(got[k], torch.cat(want_film[k], 0)), k

    whole, ranges = SA.plan_chunks(5, 256, 512), SA.plan_chunks(3, 544, 128)
    assert [nb for _, nb, _, _ in whole] == [2, 2, 1] and len(ranges) == 15 and ranges[4] == (0, 1, 512, 32) and ranges[5] == (1, 1, 0, 128)
    for weights in (True, False):
        check([whole], weights)
        check([ranges], weights)
        check([whole, ranges], weights)


@pytest.mark.parametrize("n_layers", [1, 2, 3, 4])
def test_label_head_fold_backward_is_the_gradient_of_the_fold(n_layers):
    """The label head (activation-free Linear stack, siren.py label_layer_linear; reference siren.py:1000-1012) is folded into one
    [n_lab, H] map before the kernels see it; its parameter gradients come back through written-out formulas, not through autograd.
    They are the gradient of the fold: fp64 against torch.autograd.grad, every depth the reference configures (2 and 3) and the ends."""
    from fenerf_amd.siren import autograd as SA
    g = torch.Generator().manual_seed(10 + n_layers)
    H, n = 24, 7
    dims = [(H, H)] * (n_layers - 1) + [(n, H)]
    params = [(torch.randn(o, i, dtype=torch.float64, generator=g).requires_grad_(True),
               torch.randn(o, dtype=torch.float64, generator=g).requires_grad_(True)) for o, i in dims]
    A, c = SA._fold_label_head(params)
    gA, gc = torch.randn(n, H, dtype=torch.float64, generator=g), torch.randn(n, dtype=torch.float64, generator=g)
    ref = torch.autograd.grad([A, c], [t for pair in params for t in pair], [gA, gc], allow_unused=True)
    got = SA._fold_label_head_backward(params, gA, gc)
    assert len(got) == n_layers
    for k, (dW, db) in enumerate(got):
        assert dW.shape == params[k][0].shape and db.shape == params[k][1].shape
        np.testing.assert_allclose(dW.numpy(), ref[2 * k].numpy(), rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(db.numpy(), ref[2 * k + 1].numpy(), rtol=1e-12, atol=1e-12)


def test_render_fusion_mode_is_per_thread_and_sanitised():
    """include/fenerf.h fenerf_set_render_fusion: returns the previous mode of the CALLING THREAD, unknown values mean AUTO, another thread
    keeps its own setting (no GPU needed: it only selects how later fenerf_render_forward calls are launched)."""
    import threading
    from fenerf_amd import native
    l = _lib.lib()
    prev = l.fenerf_set_render_fusion(_lib.FUSION_FORCE)
    try:
        assert prev == _lib.FUSION_AUTO
        assert l.fenerf_set_render_fusion(_lib.FUSION_OFF) == _lib.FUSION_FORCE
        assert l.fenerf_set_render_fusion(99) == _lib.FUSION_OFF            # 99 -> AUTO
        assert l.fenerf_set_render_fusion(_lib.FUSION_FORCE) == _lib.FUSION_AUTO
        seen = []
        t = threading.Thread(target=lambda: seen.append(l.fenerf_set_render_fusion(_lib.FUSION_OFF)))
        t.start(); t.join()
        assert seen == [_lib.FUSION_AUTO]                                    # the other thread started at the default ...
        assert l.fenerf_set_render_fusion(_lib.FUSION_FORCE) == _lib.FUSION_FORCE   # ... and did not touch this one
        with native.render_fusion("off"):
            assert l.fenerf_set_render_fusion(_lib.FUSION_OFF) == _lib.FUSION_OFF
        assert l.fenerf_set_render_fusion(_lib.FUSION_FORCE) == _lib.FUSION_FORCE   # restored by the context manager
    finally:
        l.fenerf_set_render_fusion(prev)


def test_film_params_beyond_the_init_range_are_what_the_fixtures_record():
    """procedural.film_params(phase_rev, freq0_gain): defaults unchanged bit for bit (every earlier fixture depends on them); the
    extensions add uniform phase shifts of +-phase_rev revolutions and scale the first layer's effective frequency 15 f + 30."""
    spec = proc.model_spec("texture", hidden_dim=32, grid_size=4, z_dim=8)
    base = proc.film_params(spec, 2, seed=3)
    same = proc.film_params(spec, 2, seed=3, phase_rev=0.0, freq0_gain=1.0)
    assert all(np.array_equal(base[k], same[k]) for k in base)
    big = proc.film_params(spec, 2, seed=3, phase_rev=300.0, freq0_gain=4.0)
    assert np.array_equal(big["freq_app"], base["freq_app"]) and np.array_equal(big["freq_geo"][:, 32:], base["freq_geo"][:, 32:])
    np.testing.assert_allclose(15.0 * big["freq_geo"][:, :32] + 30.0, 4.0 * (15.0 * base["freq_geo"][:, :32] + 30.0), rtol=2e-6)
    for k in ("phase_geo", "phase_app"):
        shift = (big[k] - base[k]) / (2 * np.pi)
        assert np.abs(shift).max() <= 300.0 and np.abs(shift).max() > 250.0 and abs(shift.mean()) < 30.0


def test_image_layout_function_cpu_bits():
    """ImageLayoutFunction (the generators' NCHW * 2 - 1 epilogue as one op each way) against the reference's three ops, bit for bit"""
    import torch
    from fenerf_amd.generators.autograd import ImageLayoutFunction
    torch.manual_seed(0)
    px = torch.rand(2, 8 * 8, 21, requires_grad=True)
    w = torch.randn(2, 21, 8, 8)
    out = ImageLayoutFunction.apply(px, 2, 8)
    ref = px.reshape(2, 8, 8, -1).permute(0, 3, 1, 2).contiguous() * 2 - 1
    assert out.is_contiguous() and torch.equal(out, ref)
    g, = torch.autograd.grad((out * w).sum(), px)
    g_ref, = torch.autograd.grad((ref * w).sum(), px)
    assert torch.equal(g, g_ref)


def test_label_head_backward_validates_before_any_launch():
    """fenerf_label_head_backward: argument errors are reported without touching a device"""
    import ctypes as C
    from fenerf_amd import _lib
    l = _lib.lib()
    assert l.fenerf_label_head_workspace_floats(256) == (2 * 32 + 1) * 256 and l.fenerf_label_head_workspace_floats(0) == 0
    null = (C.c_void_p * 3)()
    assert l.fenerf_label_head_backward(4, 256, 18, null, null, None, None, null, null, None, None) == _lib.E_INVALID
    assert b"n_layers" in l.fenerf_last_error()
    assert l.fenerf_label_head_backward(2, 256, 33, null, null, None, None, null, null, None, None) == _lib.E_INVALID
    assert b"n_lab <= 32" in l.fenerf_last_error()
    assert l.fenerf_label_head_backward(2, 256, 18, null, null, None, None, null, null, None, None) == _lib.E_INVALID
    assert b"NULL" in l.fenerf_last_error()


@pytest.mark.parametrize("softmax_label,dtype", [(True, "float32"), (False, "float32"), (False, "float16"), (True, "float64")])
def test_finish_scaled_fallback_is_the_references_epilogue(softmax_label, dtype):
    """_Generator3dBase._finish_scaled away from the one-launch device path (softmax_label=True, host tensors, non-fp32 pixels) is the
    reference's epilogue statement for statement (generators/generators.py:520-525, :97-102): softmax over the label channels, NHWC ->
    NCHW, * 2 - 1.  Round 5 shipped this branch calling itself (RecursionError)."""
    import torch
    from fenerf_amd.generators import generators as G
    from fenerf_amd.siren import siren as S_
    gen = G.DoubleImplicitGenerator3d(lambda **kw: S_.TextureEmbeddingPiGAN128SEMANTICDISENTANGLE(hidden_dim=32, **kw), 16, 16, 22, softmax_label=softmax_label)
    torch.manual_seed(1)
    px = torch.rand(2, 8 * 8, 21).to(getattr(torch, dtype)).requires_grad_(True)
    out = gen._finish_scaled(px, 2, 8)
    ref = px
    if softmax_label:
        ref = torch.cat([torch.nn.Softmax(dim=-1)(px[..., :-3]), px[..., -3:]], dim=-1)
    ref = ref.reshape((2, 8, 8, -1)).permute(0, 3, 1, 2).contiguous() * 2 - 1
    assert out.shape == (2, 21, 8, 8) and out.dtype == px.dtype and out.is_contiguous() and torch.equal(out, ref)
    g, = torch.autograd.grad(out.float().square().sum(), px)
    assert torch.isfinite(g).all()
    single = G.ImplicitGenerator3d(lambda **kw: S_.SPATIALSIRENBASELINE(hidden_dim=32, **kw), 16, 4, softmax_label=softmax_label)
    assert torch.equal(single._finish_scaled(px, 2, 8), ref)


def test_bench_last_stdout_line_is_compact_and_parses_from_a_tail():
    """bench.py's contract line (round 5's grew to 20.6 KB and the driver recorded `parsed: null`): compact_line() of a full result
    object -- round 5's own, every leg present -- is one line below 4 KB that carries the contract's keys with flat `roofline` /
    `cpu_baseline` objects, survives an 8 KB tail cut of the process's stdout, and stays small whatever the legs contain."""
    import json
    import bench
    log = os.path.join(ROOT, "profiles", "r05_bench_default_command.json.log")
    full = [json.loads(l) for l in open(log).read().splitlines() if l.startswith("{")][-1]
    assert len(json.dumps(full)) > 20000                                   # the object that broke the driver's parse
    line = bench.compact_line(full)
    assert "\n" not in line and len(line.encode()) < 4096 == bench.COMPACT_LINE_LIMIT
    stdout = "RCCL version : 2.26.6\n" + json.dumps({"noise": "x" * 30000}) + "\n" + line + "\n"
    tail = stdout.encode()[-8192:].decode()
    got = json.loads(tail.rstrip("\n").splitlines()[-1])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
              "config", "roofline", "cpu_baseline"):
        assert k in got, k
    assert got["value"] == pytest.approx(full["value"], rel=1e-5) and got["config"]["workload"].startswith("configs[1]")
    roof = got["roofline"]
    assert {"bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "kernel_ms"} <= set(roof) and len(roof) <= 14
    assert all(not isinstance(v, (dict, list)) for v in roof.values())
    assert roof["frac"] == pytest.approx(roof["achieved"] / roof["peak"], rel=1e-4)
    assert {"value", "unit", "cores", "kind", "sample"} <= set(got["cpu_baseline"])
    assert got["gstep"]["ms"] == pytest.approx(full["gstep"]["ms"], rel=1e-5) and got["gstep_b6"]["ms"] > 0 and got["gstep_ddp"]["ms"] > 0
    assert "render_one_launch" not in got and "f16x2" not in got and got["detail"] == bench.DETAIL_FILE
    # legs that failed, with long messages; legs that are missing; a result with no legs at all
    broken = dict(full, gstep={"error": "RuntimeError: " + "y" * 5000}, f32={"error": "z" * 5000})
    del broken["gstep_b6"], broken["sweep64"]
    l2 = json.loads(bench.compact_line(broken))
    assert len(l2["gstep"]["error"]) <= 120 and "gstep_b6" not in l2
    bare = {k: full[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                                 "dtype", "data", "config", "roofline")}
    l3 = json.loads(bench.compact_line(bare))
    assert "cpu_baseline" not in l3 and l3["roofline"]["frac"] == pytest.approx(full["roofline"]["frac"], rel=1e-5)


def test_bench_dump_outputs_whole_or_a_seeded_sample_under_the_limit(tmp_path):
    """bench.py --dump-outputs: the last step's per-ray arrays as float32 .npy, whole while they fit; beyond the limit the same seeded
    sample of rays from every array (ray_index.npy names them), the same from run to run, within the limit."""
    import torch
    import bench
    g = torch.Generator().manual_seed(0)
    rgb, depth = torch.rand(2, 1000, 22, generator=g), torch.rand(2, 1000, generator=g)
    bench.dump_outputs(str(tmp_path / "whole"), {"rgb": rgb, "depth": depth})
    assert sorted(os.listdir(tmp_path / "whole")) == ["depth.npy", "rgb.npy"]
    assert np.array_equal(np.load(tmp_path / "whole" / "rgb.npy"), rgb.numpy()) and np.load(tmp_path / "whole" / "depth.npy").dtype == np.float32
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), {"rgb": rgb, "depth": depth}, limit=20000)
    a = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in ("rgb", "depth", "ray_index")}
    b = {n: np.load(tmp_path / "b" / (n + ".npy")) for n in ("rgb", "depth", "ray_index")}
    assert all(np.array_equal(a[n], b[n]) for n in a) and a["ray_index"].dtype == np.float64
    ix = a["ray_index"].astype(np.int64)
    assert len(ix) > 100 and np.all(np.diff(ix) > 0) and sum(v.nbytes for v in a.values()) <= 20000
    assert np.array_equal(a["rgb"], rgb.reshape(-1, 22).numpy()[ix]) and np.array_equal(a["depth"], depth.reshape(-1).numpy()[ix])
    assert bench.DUMP_LIMIT_BYTES + 3 * 4096 <= 64 * 10 ** 6


def test_bench_cpu_baseline_is_the_torch_oracle_on_all_cores(monkeypatch):
    """bench.cpu_baseline times oracle/fenerf_oracle_torch.py (every pass on torch's thread pool) under set_num_threads(all cores),
    restores the caller's thread count and honours its time budget; tiny model, 8x8 .. 128x128 replaced by a stub clock-free check of the
    bookkeeping on a small spec."""
    import torch
    import bench
    from fenerf_amd import procedural as proc
    spec = proc.model_spec("texture", hidden_dim=32, grid_size=8)
    sd = proc.make_state_dict(spec, seed=0, sigma_gain=20.0, with_mapping=False)
    film = proc.film_params(spec, 1, seed=3)
    torch.set_num_threads(2)
    seen = []
    real = bench._oracle_torch_run

    def spy(spec_, tsd, film_, S, N, hier, seed, mbs):
        seen.append((S, N, hier, mbs, torch.get_num_threads()))
        return real(spec_, tsd, film_, 16 if S == 128 else 8, 6, hier, seed, mbs)      # the shapes' bookkeeping at a size that runs in milliseconds
    monkeypatch.setattr(bench, "_oracle_torch_run", spy)
    monkeypatch.setattr(bench, "_oracle_run", lambda *a: 0.25)
    out = bench.cpu_baseline(spec, sd, film, 7, full=True)
    assert torch.get_num_threads() == 2
    cores = bench.effective_host_cores()
    assert 1 <= cores <= os.cpu_count()
    assert out["kind"] == "port" and out["cores"] == cores and out["threads"] == cores and out["unit"] == "rays/s"
    assert "elementwise ops 1" not in out["sample"] and "torch-CPU oracle" in out["sample"]
    assert [r["shape"].split(":")[0] for r in out["runs"]] == ["configs[1]", "configs[0]", "scaling batch"]
    assert all(len(r["seconds"]) == 3 for r in out["runs"]) and out["value"] == out["runs"][0]["rays_per_s"]
    assert all(t == cores for *_, t in seen) and {m for _, _, _, m, _ in seen} == {2400000, 50000}
    assert out["numpy_oracle"]["seconds"] == 0.25
    seen.clear()
    quick = bench.cpu_baseline(spec, sd, film, 7, full=False)
    assert len(quick["runs"]) == 1 and len(quick["runs"][0]["seconds"]) == 1 and len(seen) == 2
    spent = bench.cpu_baseline(spec, sd, film, 7, full=True, budget_s=0.0)
    assert len(spent["runs"][0]["seconds"]) == 1 and all("skipped" in r for r in spent["runs"][1:]) and "numpy_oracle" not in spent


def test_sparse_backward_launch_groups():
    """generators/autograd.py plan_sparse_groups: the exact-sparsity backward pads the images of a launch group to the group's fullest image;
    the plan is a partition of the batch, every group's cap is its largest member's, and it never costs more (rounds of 128-point workgroups
    over the CUs + 0.6 per group) than one group for everything or one group per image."""
    from fenerf_amd.generators.autograd import plan_sparse_groups
    cost = lambda groups, n_cus=256: sum(-(-(len(g) * c) // (128 * n_cus)) + 0.6 for g, c in groups)
    assert plan_sparse_groups([133184]) == [([0], 133184)]
    assert plan_sparse_groups([4096] * 6) == [(list(range(6)), 4096)]                                  # similar images: one group
    full = plan_sparse_groups([32, 786432, 64, 32, 96, 32])                                           # one dense image among empty ones
    assert full == [([1], 786432), ([0, 2, 3, 4, 5], 96)]
    assert plan_sparse_groups([32, 786432, 64], n_cus=1, group_cost=0.0) == [([1], 786432), ([0, 2], 64)]
    rng = np.random.default_rng(3)
    for _ in range(200):
        B = int(rng.integers(1, 13))
        caps = [int(c) * 32 for c in rng.integers(1, 24577, B)]
        n_cus = int(rng.choice([1, 8, 256]))
        groups = plan_sparse_groups(caps, n_cus)
        assert sorted(b for g, _ in groups for b in g) == list(range(B))
        assert all(c == max(caps[b] for b in g) and g == sorted(g) for g, c in groups)
        assert cost(groups, n_cus) <= min(cost([(list(range(B)), max(caps))], n_cus), cost([([b], caps[b]) for b in range(B)], n_cus)) + 1e-9


def test_image_writer_numpy_path_equals_the_torch_statements():
    """imageio_lite.make_grid / to_uint8_hwc run in numpy float32 (single-threaded: robust against CPU-quota containers, tools/exp/
    dump_timing.py); bit for bit what the torch statements they replaced computed (torchvision 0.9's make_grid / save_image arithmetic)."""
    import math
    from fenerf_amd import imageio_lite as io

    def old_grid(tensor, nrow=8, padding=2, normalize=False, value_range=None, pad_value=0.0):
        t = torch.as_tensor(tensor).detach().float().cpu()
        if t.dim() == 2:
            t = t.unsqueeze(0)
        if t.dim() == 3:
            t = t.unsqueeze(0)
        if t.shape[1] == 1:
            t = t.repeat(1, 3, 1, 1)
        if normalize:
            t = t.clone()
            low, high = (float(value_range[0]), float(value_range[1])) if value_range is not None else (float(t.min()), float(t.max()))
            t = (t.clamp(low, high) - low) / max(high - low, 1e-5)
        B, C, H, W = t.shape
        if B == 1:
            return t[0]
        xmaps = min(nrow, B)
        ymaps = int(math.ceil(B / xmaps))
        hh, ww = H + padding, W + padding
        grid = torch.full((C, hh * ymaps + padding, ww * xmaps + padding), float(pad_value))
        for k in range(B):
            y, x = divmod(k, xmaps)
            grid[:, y * hh + padding: y * hh + padding + H, x * ww + padding: x * ww + padding + W] = t[k]
        return grid

    old_u8 = lambda g: g.mul(255).add(0.5).clamp(0, 255).permute(1, 2, 0).to(torch.uint8).numpy()
    g = torch.Generator().manual_seed(0)
    for shape, kw in (((3, 33, 29), dict(normalize=True, value_range=(-1, 1))), ((5, 3, 16, 16), dict(normalize=True)),
                      ((7, 1, 9, 11), dict(nrow=3, padding=1, pad_value=0.3)), ((25, 3, 8, 8), dict(nrow=5, normalize=True, value_range=(-1, 1))),
                      ((12, 12), dict()), ((2, 3, 5, 5), dict(normalize=True, value_range=(0.25, 0.25)))):
        t = torch.randn(shape, generator=g) * 1.3
        a, b = old_grid(t, **kw), io.make_grid(t, **kw)
        assert torch.equal(a, b) and np.array_equal(old_u8(a), io.to_uint8_hwc(b)), (shape, kw)


def test_respect_cpu_quota_caps_torch_threads(monkeypatch):
    """fenerf_amd/host.py: the cores a process may use = min(logical CPUs, affinity, cgroup quota); respect_cpu_quota() lowers torch's intra-op
    thread count to it (never raises it) -- what the command-line front ends call first, since a pool sized by the logical CPU count makes
    every small CPU tensor operation cost milliseconds in a quota-limited container."""
    from fenerf_amd import host
    n = host.effective_host_cores()
    assert 1 <= n <= (os.cpu_count() or 1)
    before = torch.get_num_threads()
    try:
        monkeypatch.setattr(host, "effective_host_cores", lambda: 1)
        assert host.respect_cpu_quota() == 1 and torch.get_num_threads() == 1
        monkeypatch.setattr(host, "effective_host_cores", lambda: 10 ** 6)
        assert host.respect_cpu_quota() == 1                      # never raised
    finally:
        torch.set_num_threads(before)
