#!/usr/bin/env python
"""The two measurements of profiles/r20_free_camera.md, on the bench field (bench.py's model: texture, H = 256, 96^3 grid, sigma_gain
2000; FiLM parameters of seed 0).

  frame      one 256^2 x 48+48 no-grad frame: forward_with_frequencies (the angle route, measured first: the yardstick) and
             forward_camera_with_frequencies with Camera.from_angles of the same pose; five repeats each, a repeat = the host clock around
             10 frames ending in a device synchronise;
  inversion  callers.inverse_render at 128^2, 24+24 (hierarchical), optimize_pose=True with pose_model "angles" and "se3": ms per
             iteration (host clock around 10 iterations, three repeats), the launches of one iteration per phase
             (fenerf_phase_times), and fenerf_camera_grads alone (hipEvents around 20 calls, best of 3).

    python tools/time_free_camera.py [--steps frame inversion]
"""
import argparse
import functools
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--steps", nargs="+", default=["frame", "inversion"], choices=["frame", "inversion"])
opt = ap.parse_args()

import ctypes as C  # noqa: E402

import torch  # noqa: E402

sys.path.insert(0, ROOT)
from fenerf_amd import _lib, callers, native, procedural as proc  # noqa: E402
from fenerf_amd.camera import Camera  # noqa: E402
from fenerf_amd.generators import generators as G  # noqa: E402
from fenerf_amd.siren import siren as S_  # noqa: E402

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
    for p in gen.parameters():
        p.requires_grad_(False)
    film = {k: torch.as_tensor(v, device=dev) for k, v in proc.film_params(spec, 1, seed=0).items()}
    return gen, (film["freq_geo"], film["freq_app"], film["phase_geo"], film["phase_app"])


def clock_ms(fn, n=10):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def phase_counts(fn):
    l = _lib.lib()
    ms, calls = (C.c_double * _lib.N_PHASES)(), (C.c_int * _lib.N_PHASES)()
    torch.cuda.synchronize()
    l.fenerf_phase_timing(1)
    l.fenerf_phase_times(ms, calls, _lib.N_PHASES)        # drain
    fn()
    torch.cuda.synchronize()
    l.fenerf_phase_times(ms, calls, _lib.N_PHASES)
    l.fenerf_phase_timing(0)
    return {l.fenerf_phase_name(i).decode(): (calls[i], ms[i]) for i in range(_lib.N_PHASES) if calls[i]}


gen, film = bench_generator()
hv = math.pi / 2
render = dict(ray_start=0.88, ray_end=1.12, hierarchical_sample=True, clamp_mode="relu", nerf_noise=0, last_back=False)

if "frame" in opt.steps:
    S, N = 256, 48
    cam = Camera.from_angles(hv + 0.25, hv, 12, (S, S), device=dev)
    with torch.no_grad():
        angle = lambda: gen.forward_with_frequencies(*film, img_size=S, fov=12, num_steps=N, h_stddev=0, v_stddev=0, h_mean=hv + 0.25, v_mean=hv,
                                                     sample_dist=None, **render)
        camera = lambda: gen.forward_camera_with_frequencies(*film, cam, num_steps=N, **render)
        angle(), camera()
        a = [clock_ms(angle) for _ in range(5)]
        c = [clock_ms(camera) for _ in range(5)]
    f = lambda ts: " ".join("%.3f" % t for t in ts)
    print(f"256^2 x 48+48 no-grad frame, ms per frame (5 repeats of 10 frames): forward_with_frequencies {f(a)} (min {min(a):.3f} max {max(a):.3f}); "
          f"forward_camera_with_frequencies {f(c)} (min {min(c):.3f} max {max(c):.3f})", flush=True)

if "inversion" in opt.steps:
    S, N = 128, 24
    opts = dict(img_size=S, fov=12, num_steps=N, h_stddev=0, v_stddev=0, h_mean=torch.tensor(hv, device=dev), v_mean=torch.tensor(hv, device=dev),
                sample_dist=None, **render)
    with torch.no_grad():
        target = gen.forward_with_frequencies(*film, **dict(opts, h_mean=hv + 0.1))[0]
    for model in ("angles", "se3"):
        run = lambda n: callers.inverse_render(gen, target[:, -3:], target[:, :-3], opts, n_iterations=n, z_dim=8, n_mean_latents=16,
                                               optimize_pose=True, pose_model=model)
        run(2)
        ts = [clock_ms(lambda: run(10), n=1) / 10 for _ in range(3)]
        two, one = phase_counts(lambda: run(2)), phase_counts(lambda: run(1))
        per_iter = {k: (two[k][0] - one.get(k, (0, 0))[0]) for k in two}
        print(f"inverse_render 128^2 x 24+24, pose_model={model}: ms per iteration {' '.join('%.2f' % t for t in ts)} (set-up included, 10 iterations per "
              f"repeat); native launch groups per iteration by phase {per_iter}, {sum(per_iter.values())} in all", flush=True)
    R = S * S
    cam = Camera.from_angles(hv, hv, 12, (S, S), device=dev)
    d_o, d_d = torch.randn((1, R, 3), device=dev), torch.randn((1, R, 3), device=dev)
    ws = torch.empty(int(_lib.lib().fenerf_camera_grads_workspace_bytes(1, R)), dtype=torch.uint8, device=dev)
    call = lambda: native.camera_grads(cam.cam2world, cam.intrinsics, (S, S), None, d_o, d_d, workspace=ws)
    call()
    best = float("inf")
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            call()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / 20)
    print(f"fenerf_camera_grads alone, {R} rays (two launches, outputs' allocation included): {best * 1e3:.1f} us per call (hipEvents around 20 calls, "
          f"best of 3); chain length L({R}) = {native.camera_grads_chain_length(R)}", flush=True)
