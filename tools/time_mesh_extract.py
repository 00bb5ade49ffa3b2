#!/usr/bin/env python
"""hipEvent times of fenerf_mesh_count / fenerf_mesh_emit on the sigma lattice of one seed of the bench field (bench.py's model: texture,
H = 256, 96^3 grid, sigma_gain 2000; FiLM parameters of seed 0; the cube is the feature grid's box), and of the SIREN launch that made the
lattice -- profiles/r11_mesh_extract.md.

    python tools/time_mesh_extract.py [voxel_resolution = 256]
"""
import ctypes as C
import os
import sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fenerf_amd import _lib, callers, native, procedural as proc

dev = "cuda:0"
N = int(sys.argv[1]) if len(sys.argv) > 1 else 256
spec = proc.model_spec("texture", hidden_dim=256, grid_size=96)
sd = proc.make_state_dict(spec, seed=0, sigma_gain=2000.0, with_mapping=False)
nat = native.NativeModel(sd, spec, dev, "f16x3")
film = proc.film_params(spec, 1, seed=0)
fg, pg, fa, pa = (torch.as_tensor(film[k], device=dev) for k in ("freq_geo", "phase_geo", "freq_app", "phase_app"))
samples, origin, size = callers.create_samples(N, (0, 0, 0), 0.24, device=dev)
ev = lambda: torch.cuda.Event(enable_timing=True)
def timed(fn, reps=5):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = ev(), ev()
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return ts
out = {}
def siren():
    out["o"] = nat.siren_forward(samples, None, fg, pg, fa, pa)
t_siren = timed(siren, 3)
vol = out.pop("o")[..., -1].reshape(N, N, N).contiguous()
lo, hi, med = float(vol.min()), float(vol.max()), float(vol.median())
l = _lib.lib()
ws = torch.empty(l.fenerf_mesh_workspace_bytes(N, N, N), dtype=torch.uint8, device=dev)
counts = torch.zeros(2, dtype=torch.int64, device=dev)
p = lambda t: C.c_void_p(t.data_ptr())
o3 = (C.c_float * 3)(float(origin[2]), float(origin[1]), float(origin[0])); s3 = (C.c_float * 3)(size, size, size)
print(f"N={N} sigma in [{lo:.4g}, {hi:.4g}] median {med:.4g}; workspace {ws.numel()} bytes ({ws.numel() / N**3:.3f} per point); siren launch ms {['%.3f' % t for t in t_siren]}", flush=True)
for iso in (10.0, med):
    t_count = timed(lambda: _lib.check(l.fenerf_mesh_count(p(vol), N, N, N, iso, p(ws), p(counts), None)))
    nv, nf = (int(x) for x in counts.cpu())
    v = torch.empty((max(nv, 1), 3), dtype=torch.float32, device=dev); f = torch.empty((max(nf, 1), 3), dtype=torch.int32, device=dev)
    t_emit = timed(lambda: _lib.check(l.fenerf_mesh_emit(p(vol), N, N, N, iso, o3, s3, p(ws), nv, nf, p(v), p(f), None)))
    print(f"iso={iso:.4g}: V={nv} F={nf}; count ms {['%.3f' % t for t in t_count]}; emit ms (incl. its 16-byte host read) {['%.3f' % t for t in t_emit]}", flush=True)
    a = native.mesh_from_volume(vol, iso, (origin[2], origin[1], origin[0]), (size,) * 3)
    assert torch.equal(a[0], v[:nv]) and torch.equal(a[1], f[:nf])
    if nf:
        e = torch.cat([a[1][:, [0, 1]], a[1][:, [1, 2]], a[1][:, [2, 0]]]).long()
        key, rkey = e[:, 0] * nv + e[:, 1], e[:, 1] * nv + e[:, 0]
        unpaired = int((~torch.isin(key, rkey)).sum())
        print(f"   faces index 0..{int(a[1].max())}; directed edges {key.numel()}, unique {torch.unique(key).numel()}, without a reverse {unpaired} (open only at the volume's boundary)", flush=True)
