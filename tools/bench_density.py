#!/usr/bin/env python
"""Times of the geometry route (density and labels without the colour branch) against the full forward on the bench field (bench.py's
model: texture, H = 256, 96^3 grid, sigma_gain 2000; FiLM parameters of seed 0) -- profiles/r18_density_route.md.  Three pairs, the two
sides of each alternated `--rounds` times in one process:

  query   fenerf_siren_density (sigma alone) / fenerf_siren_forward over N^3 lattice points, hipEvents around `--iters` back-to-back calls
  lattice callers.sample_generator at N^3 end to end (wall clock, the volume on the host), density route / full-forward route (the route of
          a model that does not serve the density query: the statements the caller had before the route existed)
  render  fenerf_render_density / fenerf_render_forward at S^2 rays, K + K samples, hipEvents around `--iters` back-to-back calls

    python tools/bench_density.py [--resolution 256] [--image_size 256] [--num_steps 48] [--rounds 5] [--iters 5]

One JSON line per pair: medians, min - max of each side, the ratio of the medians."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fenerf_amd import _lib, callers, native, procedural as proc  # noqa: E402
from fenerf_amd.generators import generators as G  # noqa: E402
from fenerf_amd.generators import volumetric_rendering as VR  # noqa: E402
from fenerf_amd.siren import siren as S_  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--image_size", type=int, default=256)
    ap.add_argument("--num_steps", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    opt = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    spec = proc.model_spec("texture", hidden_dim=256, grid_size=96, z_dim=8)
    sd = proc.make_state_dict(spec, seed=0, sigma_gain=2000.0, with_mapping=False)
    torch.manual_seed(0)
    mod = S_.TextureEmbeddingPiGAN128SEMANTICDISENTANGLE(hidden_dim=256, z_geo_dim=8, z_app_dim=8, output_dim=22)
    tsd = {k: torch.from_numpy(v) for k, v in sd.items()}
    mod.spatial_embeddings = torch.nn.Parameter(tsd["spatial_embeddings"].clone())
    mod.load_state_dict(tsd, strict=False)
    mod.precision = "f16x3"
    mod = mod.to(dev)
    mod.device = dev
    gen = G.DoubleImplicitGenerator3d(lambda **kw: mod, 8, 8, 22)
    gen.siren = mod
    gen = gen.to(dev).eval()
    gen.device = dev
    nat = mod.native(dev)
    assert nat.supports_density()
    film = proc.film_params(spec, 1, seed=0)
    fg, pg, fa, pa = (torch.as_tensor(film[k], device=dev) for k in ("freq_geo", "phase_geo", "freq_app", "phase_app"))

    def events(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(opt.iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / opt.iters

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def pair(name, new, old, timer, **extra):
        new(), old()                        # warm-up: allocations, LDS opt-in, the cached average frequencies
        torch.cuda.synchronize()
        t_new, t_old = [], []
        for _ in range(opt.rounds):         # alternated
            t_old.append(timer(old))
            t_new.append(timer(new))
        side = lambda ts: dict(median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4))
        print(json.dumps(dict(pair=name, density=side(t_new), full=side(t_old), ratio=round(statistics.median(t_new) / statistics.median(t_old), 4),
                              full_spread_ms=round(max(t_old) - min(t_old), 4), gain_ms=round(statistics.median(t_old) - statistics.median(t_new), 4),
                              rounds=opt.rounds, **extra)), flush=True)

    # ---- query
    N = opt.resolution
    samples, _, _ = callers.create_samples(N, (0, 0, 0), 0.24, device=dev)
    sigma = torch.empty((1, N ** 3), dtype=torch.float32, device=dev)
    keep = {}
    pair("query", lambda: nat.siren_density(samples, fg, pg, labels=False, out=sigma),
         lambda: keep.__setitem__("o", nat.siren_forward(samples, None, fg, pg, fa, pa)), events, points=N ** 3, iters=opt.iters)
    assert torch.equal(sigma[0], keep["o"][0, :, -1])
    keep.clear()
    torch.cuda.empty_cache()
    # ---- lattice
    z = torch.randn(1, 8, device=dev)
    vols = {}

    def lattice(route):
        def run():
            torch.manual_seed(1)
            if route == "full":
                real = native.NativeModel.supports_density
                native.NativeModel.supports_density = lambda self: False
                try:
                    vols[route] = callers.sample_generator(gen, z, voxel_resolution=N, cube_length=0.24)
                finally:
                    native.NativeModel.supports_density = real
            else:
                vols[route] = callers.sample_generator(gen, z, voxel_resolution=N, cube_length=0.24)
        return run
    pair("lattice", lattice("density"), lattice("full"), wall, points=N ** 3)
    assert np.array_equal(vols["density"].view(np.uint32), vols["full"].view(np.uint32))
    vols.clear()
    del samples, sigma
    torch.cuda.empty_cache()
    # ---- render
    S, K = opt.image_size, opt.num_steps
    torch.manual_seed(0)
    o, d, zc, _, _ = VR.sample_rays(1, K, dev, 12, (S, S), 0.88, 1.12, 0.3, 0.155, np.pi / 2, np.pi / 2, "gaussian")
    u = torch.rand((S * S, K), device=dev)
    opts = _lib.composite_opts("relu", 0.0, fill_mode="seg_padding_background", fill_color="black")
    out = {}
    pair("render", lambda: out.__setitem__("d", nat.render_density(o, d, zc, u, None, None, fg, pg, opts)),
         lambda: out.__setitem__("f", nat.render(o, d, zc, u, None, None, fg, pg, fa, pa, opts)), events, rays=S * S, samples=[K, K], iters=opt.iters)
    assert torch.equal(out["d"][0], out["f"][0][..., :-3]) and torch.equal(out["d"][1], out["f"][1])


if __name__ == "__main__":
    main()
