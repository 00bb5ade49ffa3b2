"""fenerf_composite_backward_outputs (the depth / weights / wsum variant of the composite backward) against fenerf_composite_backward on
the same rays: device time per launch, interleaved A / B, median over rounds of batched launches between two events.

    python tools/exp/composite_backward_outputs_timing.py [--rays 16384] [--N 24] [--C 22] [--rounds 30] [--batch 20]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from fenerf_amd import _lib, native          # noqa: E402

DEV = "cuda:0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=128 * 128)
    ap.add_argument("--N", type=int, default=24)
    ap.add_argument("--C", type=int, default=22)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--batch", type=int, default=20)
    a = ap.parse_args()
    BR, N, C = a.rays, a.N, a.C
    g = torch.Generator(device=DEV).manual_seed(0)
    rn = lambda *s: torch.randn(s, device=DEV, generator=g)
    res = {"config": {"rays": BR, "N": N, "C": C, "rounds": a.rounds, "batch": a.batch}}
    for merge in (True, False):
        M = 2 * N if merge else N
        rows_a, rows_b = rn(BR, N, C), (rn(BR, N, C) if merge else None)
        for r in (rows_a, rows_b):
            if r is not None:
                r[..., -1] *= 20
        z_a = torch.sort(torch.rand((BR, N), device=DEV, generator=g) * 0.24 + 0.88, -1)[0]
        z_b = torch.sort(torch.rand((BR, N), device=DEV, generator=g) * 0.24 + 0.88, -1)[0] if merge else None
        noise, g_rgb, g_depth, g_w, g_ws = rn(BR, M), rn(BR, C - 1), rn(BR), rn(BR, M), rn(BR)
        opts = _lib.composite_opts("relu", 0.2)
        out_a, out_b = torch.empty_like(rows_a), (torch.empty_like(rows_b) if merge else None)
        common = dict(rows_b=rows_b, z_b=z_b, noise=noise, out_a=out_a, out_b=out_b)
        variants = {"rgb (fenerf_composite_backward)": lambda: native.composite_backward(g_rgb, rows_a, z_a, opts, **common),
                    "rgb + depth": lambda: native.composite_backward(g_rgb, rows_a, z_a, opts, g_depth=g_depth, **common),
                    "depth only": lambda: native.composite_backward(None, rows_a, z_a, opts, g_depth=g_depth, **common),
                    "rgb + depth + weights + wsum": lambda: native.composite_backward(g_rgb, rows_a, z_a, opts, g_depth=g_depth, g_weights=g_w,
                                                                                      g_wsum=g_ws, **common)}
        times = {k: [] for k in variants}
        for fn in variants.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for k, fn in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.batch):
                    fn()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) / a.batch * 1e3)
        res["merge" if merge else "single"] = {k: {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
                                               for k, v in times.items()}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
