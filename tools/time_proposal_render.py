#!/usr/bin/env python
"""What the proposal lattice costs and how close its frames are to the exact ones -- profiles/r19_proposal_render.md.

Four steps, each a process of its own under its own time limit (the driver stops at the first step that fails or runs out of time):
  bake      callers.bake_density of the bench field (bench.py's model: texture, H = 256, 96^3 grid, sigma_gain 2000; FiLM parameters of seed 0)
            at 128^3 / 256^3 / 384^3 / 512^3: ms (second call, host clock around the call and a synchronise) and lattice bytes;
  frames    per-frame host clocks (10 frames ending in a device synchronise, three rounds with the legs alternating) at 128^2 x 24+24 and
            256^2 x 48+48: exact staged_forward_with_frequencies, DensityField.render (256^3) with lock_view_dependence False and True,
            BakedField.render (256^3);
  kernels   hipEvent times of fenerf_render_proposal alone and of fenerf_proposal_depths alone on the rays of one view;
  fidelity  PSNR over rgb (range 2), max abs rgb and label agreement of DensityField.render against the exact render of the same seed, per
            lattice resolution, beside exact(seed a) against exact(seed b) and BakedField.render against the exact locked-view render, on the
            bench field and on tests/golden/ref_generator_tiny.pth (seed 3, psi 0.7).

    python tools/time_proposal_render.py [--steps bake frames kernels fidelity] [--skip_tiny] [--resolutions 128 256 384]
"""
import argparse
import functools
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_SECONDS = {"bake": 240, "frames": 300, "kernels": 180, "fidelity": 420}

ap = argparse.ArgumentParser()
ap.add_argument("--steps", nargs="+", default=list(STEP_SECONDS), choices=list(STEP_SECONDS))
ap.add_argument("--step", default=None, choices=list(STEP_SECONDS), help="run this one step in this process (what the driver starts)")
ap.add_argument("--skip_tiny", action="store_true")
ap.add_argument("--resolutions", type=int, nargs="+", default=[128, 256, 384])
opt = ap.parse_args()

if opt.step is None:
    for step in opt.steps:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--resolutions", *map(str, opt.resolutions)] + (["--skip_tiny"] if opt.skip_tiny else [])
        try:
            rc = subprocess.run(cmd, timeout=STEP_SECONDS[step]).returncode
        except subprocess.TimeoutExpired:
            raise SystemExit(f"step {step}: no result within {STEP_SECONDS[step]} s; stopping")
        if rc != 0:
            raise SystemExit(f"step {step}: exit status {rc}; stopping")
    raise SystemExit(0)

import torch  # noqa: E402

sys.path.insert(0, ROOT)
from fenerf_amd import _lib, callers, native, procedural as proc  # noqa: E402
from fenerf_amd.generators import generators as G  # noqa: E402
from fenerf_amd.siren import siren as S_  # noqa: E402
from fenerf_amd.generators import volumetric_rendering as VR  # noqa: E402


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


dev = torch.device("cuda:0")
fmt = lambda ts: "middle %.3f of %s" % (statistics.median(ts), ["%.3f" % t for t in ts])


def view_kw(S, N, lock):
    return dict(img_size=S, fov=12, ray_start=0.88, ray_end=1.12, num_steps=N, h_stddev=0, v_stddev=0, h_mean=math.pi / 2 + 0.25, v_mean=math.pi / 2,
                hierarchical_sample=True, sample_dist=None, clamp_mode="relu", nerf_noise=0, last_back=False, fill_mode="eval_seg_padding_background",
                fill_color="black", lock_view_dependence=lock)


def film_of(meta):
    return (meta["truncated_frequencies_geo"], meta["truncated_frequencies_app"], meta["truncated_phase_shifts_geo"], meta["truncated_phase_shifts_app"])


def three(a, b):
    """PSNR over rgb (range 2), max abs rgb, label agreement of two frames [1,C',S,S]"""
    rgb_a, rgb_b = a[:, -3:].double(), b[:, -3:].double()
    mse = float(((rgb_a - rgb_b) ** 2).mean())
    psnr = float("inf") if mse == 0 else 10 * math.log10(4.0 / mse)
    agree = float((a[:, :-3].argmax(1) == b[:, :-3].argmax(1)).float().mean())
    return f"{psnr:.1f} dB / {float((rgb_a - rgb_b).abs().max()):.2f} / {agree:.3f}"


gen, meta = bench_generator()
film = film_of(meta)

if opt.step == "bake":
    cube = callers.baked_cube_length(12, 0.88, 1.12, num_steps=24)
    for n in (128, 256, 384, 512):
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            field = callers.bake_density(gen, None, film=meta, resolution=n, cube_length=cube)
            torch.cuda.synchronize()
            ms = 1e3 * (time.perf_counter() - t0)
            nbytes = field.vol.numel() * 4
            positive = float((field.vol > 0).float().mean())
            del field
            torch.cuda.empty_cache()
        print(f"bench field: bake_density {n}^3 {ms:.1f} ms (second call), {nbytes} bytes ({nbytes / 2 ** 20:.0f} MiB), sigma > 0 on {positive:.3f} of the lattice", flush=True)

if opt.step == "frames":
    for S, N in ((128, 24), (256, 48)):
        cube = callers.baked_cube_length(12, 0.88, 1.12, num_steps=N)
        dens = callers.bake_density(gen, None, film=meta, resolution=256, cube_length=cube)
        baked = callers.bake_field(gen, None, film=meta, resolution=256, cube_length=cube)
        kw0, kw1 = view_kw(S, N, False), view_kw(S, N, True)
        res = legs({"exact staged_forward_with_frequencies (view-dependent)": lambda: gen.staged_forward_with_frequencies(*film, **kw0),
                      "exact staged_forward_with_frequencies (locked view)": lambda: gen.staged_forward_with_frequencies(*film, **kw1),
                      "DensityField.render 256^3 (view-dependent)": lambda: dens.render(gen, **kw0),
                      "DensityField.render 256^3 (locked view)": lambda: dens.render(gen, **kw1),
                      "BakedField.render 256^3": lambda: baked.render(gen, **kw1)})
        for k, ts in res.items():
            print(f"{S}^2 x {N}+{N}  {k}: ms per frame {fmt(ts)}", flush=True)
        del dens, baked
        torch.cuda.empty_cache()

if opt.step == "kernels":
    nat = gen.siren.native(dev)
    fg, fa, pg, pa = film
    opts = _lib.composite_opts("relu")
    for S, N in ((128, 24), (256, 48)):
        cube = callers.baked_cube_length(12, 0.88, 1.12, num_steps=N)
        dens = callers.bake_density(gen, None, film=meta, resolution=256, cube_length=cube)
        torch.manual_seed(0)
        o, d, z, _, _ = VR.sample_rays(1, N, dev, 12, (S, S), 0.88, 1.12, 0, 0, math.pi / 2 + 0.25, math.pi / 2, None)
        R = S * S
        z = z.reshape(1, R, N).contiguous()
        u = torch.rand((R, N), device=dev)
        depths = lambda: native.proposal_depths(dens.vol, dens.origin, dens.spacing, o, d, z, u, None, opts, dens.outside_last)
        render = lambda lock: nat.render_proposal(dens.vol, dens.origin, dens.spacing, o, d, z, u, None, None, fg, pg, fa, pa, opts, outside_last=dens.outside_last,
                                                  lock_view=lock)
        print(f"{S}^2 x {N} ({R} rays, 256^3 lattice)  fenerf_proposal_depths {events_ms(depths):.4f} ms, fenerf_render_proposal "
              f"{events_ms(lambda: render(False), launches=10):.3f} ms view-dependent / {events_ms(lambda: render(True), launches=10):.3f} ms locked view; "
              f"NativeModel.render (exact, two SIREN passes) {events_ms(lambda: nat.render(o, d, z, u, None, None, fg, pg, fa, pa, opts), launches=10):.3f} ms "
              f"(hipEvents around the launches, best of 3, allocation of the outputs included)", flush=True)
        del dens
        torch.cuda.empty_cache()

if opt.step == "fidelity":
    cases = [("bench field", gen, meta)]
    if not opt.skip_tiny:
        cases.append(("ref_generator_tiny.pth",) + tiny_generator())
    for name, g, m in cases:
        f = film_of(m)
        for S, N in ((128, 24), (256, 48)):
            kw0, kw1 = view_kw(S, N, False), view_kw(S, N, True)
            cube = callers.baked_cube_length(12, 0.88, 1.12, num_steps=N)
            frame = lambda fn, seed, kw: (torch.manual_seed(seed), fn(**kw)[0])[1]
            exact = lambda **kw: g.staged_forward_with_frequencies(*f, **kw)
            ex_a, ex_b, ex_lock = frame(exact, 1, kw0), frame(exact, 2, kw0), frame(exact, 1, kw1)
            print(f"{name}, {S}^2 x {N}+{N}: PSNR / max abs rgb / label agreement: exact(seed a) vs exact(seed b) {three(ex_b, ex_a)}", flush=True)
            for n in opt.resolutions:
                dens = callers.bake_density(g, None, film=m, resolution=n, cube_length=cube)
                prop = frame(lambda **kw: dens.render(g, **kw), 1, kw0)
                prop_lock = frame(lambda **kw: dens.render(g, **kw), 1, kw1)
                del dens
                baked = callers.bake_field(g, None, film=m, resolution=n, cube_length=cube)
                bk = frame(lambda **kw: baked.render(g, **kw), 1, kw1)
                del baked
                torch.cuda.empty_cache()
                print(f"{name}, {S}^2 x {N}+{N}, {n}^3: proposal vs exact {three(prop, ex_a)}; proposal vs exact, locked view {three(prop_lock, ex_lock)}; "
                      f"baked vs exact, locked view {three(bk, ex_lock)}", flush=True)
