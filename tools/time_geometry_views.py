#!/usr/bin/env python
"""What a geometry view costs and how well lattice normals agree with exact ones -- profiles/r15_geometry_views.md.

Per-frame host clocks (10 frames ending in a device synchronise, three rounds with the legs alternating) of callers.render_geometry against
staged_forward_with_frequencies (exact route) and of BakedField.render_geometry against BakedField.render (256^3 lattice), at 128^2 x 24+24 and
256^2 x 48+48 on the bench field (bench.py's model: texture, H = 256, 96^3 grid, sigma_gain 2000; FiLM parameters of seed 0); hipEvent times of
the three geometry kernels alone; and the angle between baked and exact normals over the rays visible in both at 128^3 / 256^3 / 384^3 on
the bench field and on tests/golden/ref_generator_tiny.pth (seed 3, psi 0.7).

    python tools/time_geometry_views.py [--skip_tiny] [--resolutions 128 256 384]
"""
import argparse
import functools
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fenerf_amd import callers, native, procedural as proc
from fenerf_amd.generators import generators as G
from fenerf_amd.siren import siren as S_

ap = argparse.ArgumentParser()
ap.add_argument("--skip_tiny", action="store_true")
ap.add_argument("--resolutions", type=int, nargs="+", default=[128, 256, 384])
opt = ap.parse_args()
dev = torch.device("cuda:0")


def bench_generator():
    spec = proc.model_spec("texture", hidden_dim=256, grid_size=96, z_dim=8)
    sd = proc.make_state_dict(spec, seed=0, sigma_gain=2000.0, with_mapping=False)
    mod = S_.TextureEmbeddingPiGAN128SEMANTICDISENTANGLE(hidden_dim=256, z_geo_dim=8, z_app_dim=8, output_dim=22)
    tsd = {k: torch.from_numpy(v) for k, v in sd.items()}
    mod.spatial_embeddings = torch.nn.Parameter(tsd["spatial_embeddings"].clone())
    mod.load_state_dict(tsd, strict=False)
    gen = G.DoubleImplicitGenerator3d(functools.partial(S_.TextureEmbeddingPiGAN128SEMANTICDISENTANGLE, hidden_dim=256), 8, 8, 22)
    gen.siren = mod
    gen = gen.to(dev).eval()
    gen.device = dev
    gen.siren.device = dev
    film = {k: torch.as_tensor(v, device=dev) for k, v in proc.film_params(spec, 1, seed=0).items()}
    return gen, dict(truncated_frequencies_geo=film["freq_geo"], truncated_phase_shifts_geo=film["phase_geo"],
                     truncated_frequencies_app=film["freq_app"], truncated_phase_shifts_app=film["phase_app"])


def tiny_generator():
    gen = callers.load_generator(os.path.join(ROOT, "tests", "golden", "ref_generator_tiny.pth"), dev, use_ema=False)
    torch.manual_seed(3)
    zg, za = callers._latent_dims(gen)
    z_geo, z_app = torch.randn((1, zg), device=dev), torch.randn((1, za), device=dev)
    avg_fg, avg_pg, avg_fa, avg_pa = gen.generate_avg_frequencies()
    with torch.no_grad():
        raw_fg, raw_pg = gen.siren.geo_mapping_network(z_geo)
        raw_fa, raw_pa = gen.siren.app_mapping_network(z_app)
    t = lambda avg, raw: avg + 0.7 * (raw - avg)
    return gen, dict(truncated_frequencies_geo=t(avg_fg, raw_fg), truncated_phase_shifts_geo=t(avg_pg, raw_pg),
                     truncated_frequencies_app=t(avg_fa, raw_fa), truncated_phase_shifts_app=t(avg_pa, raw_pa))


def view_kw(S, N):
    return dict(img_size=S, fov=12, ray_start=0.88, ray_end=1.12, num_steps=N, h_stddev=0, v_stddev=0, h_mean=math.pi / 2 + 0.25, v_mean=math.pi / 2,
                hierarchical_sample=True, sample_dist=None, clamp_mode="relu", nerf_noise=0, last_back=False, fill_mode="eval_seg_padding_background",
                fill_color="black", lock_view_dependence=True)


def frames_ms(fn, frames=10):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(frames):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / frames


def legs(named, rounds=3):
    """every leg once per round, alternating; -> {name: [ms per round]}"""
    for fn in named.values():
        fn()          # warm-up: workspaces, first-launch costs
    out = {k: [] for k in named}
    for _ in range(rounds):
        for k, fn in named.items():
            out[k].append(frames_ms(fn))
    return out


def events_ms(fn, launches=20, reps=3):
    fn()
    best = float("inf")
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b) / launches)
    return best


def angles(view_a, view_b, alpha_min=0.5):
    R = view_a["alpha"].numel()
    both = (view_a["alpha"].reshape(R) >= alpha_min) & (view_b["alpha"].reshape(R) >= alpha_min)
    na, nb = (v["normal"][0].reshape(3, R).t().double()[both] for v in (view_a, view_b))
    ang = torch.arccos(((na * nb).sum(-1)).clamp(-1, 1)).numpy()
    return int(both.sum()), R, float(ang.mean()), float(np.quantile(ang, 0.95))


fmt = lambda ts: "middle %.3f of %s" % (statistics.median(ts), ["%.3f" % t for t in ts])
gen, meta = bench_generator()
film = (meta["truncated_frequencies_geo"], meta["truncated_frequencies_app"], meta["truncated_phase_shifts_geo"], meta["truncated_phase_shifts_app"])
cube = callers.baked_cube_length(12, 0.88, 1.12, num_steps=24)
t0 = time.perf_counter()
field = callers.bake_field(gen, None, film=meta, resolution=256, cube_length=cube)
torch.cuda.synchronize()
print(f"bench field: bake 256^3 {1e3 * (time.perf_counter() - t0):.1f} ms, cube {cube:.4f}", flush=True)
for S, N in ((128, 24), (256, 48)):
    kw = view_kw(S, N)
    res = legs({"exact staged_forward_with_frequencies": lambda: gen.staged_forward_with_frequencies(*film, **kw),
                "exact render_geometry": lambda: callers.render_geometry(gen, film=meta, **kw),
                "BakedField.render 256^3": lambda: field.render(gen, **kw),
                "BakedField.render_geometry 256^3": lambda: field.render_geometry(gen, **kw)})
    for k, ts in res.items():
        print(f"{S}^2 x {N}+{N}  {k}: ms per frame {fmt(ts)}", flush=True)
    # the three kernels alone, on the rays of one view
    torch.manual_seed(0)
    view = callers.render_geometry(gen, film=meta, details=True, **kw)
    R = S * S
    o, d = view["origins"].to(dev), view["dirs"].to(dev)
    depth, alpha = view["depth"].reshape(1, R).to(dev), view["alpha"].reshape(1, R).to(dev)
    pts, grad, c2w = view["points"].to(dev), view["grad"].to(dev), view["cam2world"].to(dev)
    print(f"{S}^2 ({R} rays)  fenerf_surface_points {events_ms(lambda: native.surface_points(o, d, depth, alpha, 0.5)):.4f} ms, "
          f"fenerf_volume_sample_grad (256^3) {events_ms(lambda: native.volume_sample_grad(field.vol, field.origin, field.spacing, pts, field.C - 1)):.4f} ms, "
          f"fenerf_shade_normals {events_ms(lambda: native.shade_normals(grad, R, alpha, c2w)):.4f} ms (hipEvents around 20 launches, best of 3, allocation of the "
          f"outputs included); exact input gradient of the {pts.shape[1]} points "
          f"{events_ms(lambda: callers._sigma_input_grads(gen.siren, pts, film[0], film[2], film[1], film[3], callers.MESH_NORMAL_CHUNK), launches=5):.3f} ms", flush=True)
del field
torch.cuda.empty_cache()

cases = [("bench field", gen, meta, (128, 24))]
if not opt.skip_tiny:
    cases.append(("ref_generator_tiny.pth",) + tiny_generator() + ((128, 24),))
for name, g, m, (S, N) in cases:
    kw = view_kw(S, N)
    torch.manual_seed(1)
    exact = callers.render_geometry(g, film=m, **kw)
    vis = float((exact["alpha"] >= 0.5).float().mean())
    for n in opt.resolutions:
        field = callers.bake_field(g, None, film=m, resolution=n, cube_length=callers.baked_cube_length(12, 0.88, 1.12, num_steps=N))
        torch.manual_seed(1)
        baked = field.render_geometry(g, **kw)
        both, R, mean, p95 = angles(baked, exact)
        print(f"{name}, {S}^2 x {N}+{N}, {n}^3 lattice (spacing {field.spacing[0]:.5f}): baked vs exact normals over {both} of {R} rays visible in both "
              f"(exact visible fraction {vis:.3f}): mean angle {mean:.4f} rad ({math.degrees(mean):.2f} deg), 95th percentile {p95:.4f} rad ({math.degrees(p95):.2f} deg); "
              f"max |shaded difference| {float((baked['shaded'] - exact['shaded']).abs().max()):.3f}, mean {float((baked['shaded'] - exact['shaded']).abs().mean()):.4f}", flush=True)
        del field
        torch.cuda.empty_cache()
