#!/usr/bin/env python
"""hipEvent times of fenerf_mesh_count / fenerf_mesh_emit on the sigma lattice of one seed of the bench field (bench.py's model: texture,
H = 256, 96^3 grid, sigma_gain 2000; FiLM parameters of seed 0; the cube is the feature grid's box), and of the SIREN launch that made the
lattice -- profiles/r11_mesh_extract.md.  With --keep_largest / --min_component N / --simplify K also the mesh-cleaning calls
(fenerf_volume_components, fenerf_volume_keep_components, fenerf_mesh_cluster_count, fenerf_mesh_cluster_emit), the mesh before and after,
and the wall time of the whole callers.extract_mesh with and without the option -- profiles/r13_mesh_clean.md.  --blobs M plants M
detached 3^3 blobs of density (each inside a carved shell) into the lattice first (the kernel times only: extract_mesh evaluates the field itself).

    python tools/time_mesh_extract.py [voxel_resolution = 256] [--keep_largest] [--min_component N] [--simplify K] [--blobs M]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time
import types
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fenerf_amd import _lib, callers, native, procedural as proc
from fenerf_amd.siren import siren as S_

ap = argparse.ArgumentParser()
ap.add_argument("voxel_resolution", type=int, nargs="?", default=256)
ap.add_argument("--keep_largest", action="store_true")
ap.add_argument("--min_component", type=int, default=None)
ap.add_argument("--simplify", type=int, default=None)
ap.add_argument("--blobs", type=int, default=0)
opt = ap.parse_args()

dev = "cuda:0"
N = opt.voxel_resolution
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
frame = ((origin[2], origin[1], origin[0]), (size,) * 3)
ms = lambda ts: "median %.3f of %s" % (statistics.median(ts), ["%.3f" % t for t in ts])
print(f"N={N} sigma in [{lo:.4g}, {hi:.4g}] median {med:.4g}; workspace {ws.numel()} bytes ({ws.numel() / N**3:.3f} per point); siren launch ms {['%.3f' % t for t in t_siren]}", flush=True)
clean = opt.keep_largest or opt.min_component is not None or opt.simplify is not None
for iso in (10.0,) if clean else (10.0, med):
    t_count = timed(lambda: _lib.check(l.fenerf_mesh_count(p(vol), N, N, N, iso, p(ws), p(counts), None)))
    nv, nf = (int(x) for x in counts.cpu())
    v = torch.empty((max(nv, 1), 3), dtype=torch.float32, device=dev); f = torch.empty((max(nf, 1), 3), dtype=torch.int32, device=dev)
    t_emit = timed(lambda: _lib.check(l.fenerf_mesh_emit(p(vol), N, N, N, iso, o3, s3, p(ws), nv, nf, p(v), p(f), None)))
    print(f"iso={iso:.4g}: V={nv} F={nf}; count ms {['%.3f' % t for t in t_count]}; emit ms (incl. its 16-byte host read) {['%.3f' % t for t in t_emit]}", flush=True)
    a = native.mesh_from_volume(vol, iso, *frame)
    assert torch.equal(a[0], v[:nv]) and torch.equal(a[1], f[:nf])
    if nf:
        e = torch.cat([a[1][:, [0, 1]], a[1][:, [1, 2]], a[1][:, [2, 0]]]).long()
        key, rkey = e[:, 0] * nv + e[:, 1], e[:, 1] * nv + e[:, 0]
        unpaired = int((~torch.isin(key, rkey)).sum())
        print(f"   faces index 0..{int(a[1].max())}; directed edges {key.numel()}, unique {torch.unique(key).numel()}, without a reverse {unpaired} (open only at the volume's boundary)", flush=True)
if not clean:
    sys.exit(0)

# ---- mesh cleaning at iso = 10 -------------------------------------------------------------------------------------------------------
iso = 10.0
for name in ("v", "f", "a", "e", "key", "rkey"):
    globals().pop(name, None)
def clean_kernels(vol, tag):
    cws = torch.empty(l.fenerf_volume_components_workspace_bytes(N, N, N), dtype=torch.uint8, device=dev)
    labels = torch.empty((N, N, N), dtype=torch.int32, device=dev)
    stats = torch.zeros(4, dtype=torch.int64, device=dev)
    t_cc = timed(lambda: _lib.check(l.fenerf_volume_components(p(vol), N, N, N, iso, p(cws), p(labels), p(stats), None)))
    st = stats.cpu().tolist()
    print(f"[{tag}] components: {st[0]} inside points in {st[1]} components, the largest {st[3]} points at label {st[2]}; workspace {cws.numel()} bytes; "
          f"fenerf_volume_components ms {ms(t_cc)}", flush=True)
    v0, f0 = native.mesh_from_volume(vol, iso, *frame)
    print(f"[{tag}] unfiltered mesh: V={len(v0)} F={len(f0)}", flush=True)
    meshes = {"all": (v0, f0)}
    for name, mode, mp in (("largest", _lib.KEEP_LARGEST, 1),) * opt.keep_largest + ((f"min {opt.min_component}", _lib.KEEP_MIN_POINTS, opt.min_component),) * (opt.min_component is not None):
        kept = torch.empty_like(vol)
        t_keep = timed(lambda: _lib.check(l.fenerf_volume_keep_components(p(vol), p(labels), p(cws), N, N, N, mode, mp, p(kept), None)))
        vk, fk = native.mesh_from_volume(kept, iso, *frame)
        meshes[name] = (vk, fk)
        print(f"[{tag}] keep {name}: fenerf_volume_keep_components ms {ms(t_keep)}; mesh V={len(vk)} F={len(fk)}", flush=True)
        del kept
    if opt.simplify is not None:
        K = opt.simplify
        for name, (vm, fm) in meshes.items():
            V, F = len(vm), len(fm)
            kws = torch.empty(l.fenerf_mesh_cluster_workspace_bytes(V, F, N, N, N, K), dtype=torch.uint8, device=dev)
            c3 = torch.zeros(3, dtype=torch.int64, device=dev)
            t_c = timed(lambda: _lib.check(l.fenerf_mesh_cluster_count(p(vm), V, p(fm), F, o3, s3, N, N, N, K, p(kws), p(c3), None)))
            cv, cf, bad = c3.cpu().tolist()
            vo = torch.empty((max(cv, 1), 3), dtype=torch.float32, device=dev); fo = torch.empty((max(cf, 1), 3), dtype=torch.int32, device=dev)
            t_e = timed(lambda: _lib.check(l.fenerf_mesh_cluster_emit(p(fm), V, F, o3, s3, N, N, N, K, p(kws), cv, cf, p(vo), p(fo), None)))
            print(f"[{tag}] simplify {K} of the '{name}' mesh: V {V} -> {cv}, F {F} -> {cf}; workspace {kws.numel()} bytes; cluster_count ms {ms(t_c)}; "
                  f"cluster_emit ms (incl. its 24-byte host read) {ms(t_e)}", flush=True)
            del kws, vo, fo

clean_kernels(vol, "field")
if opt.blobs:
    rng = np.random.default_rng(0)
    planted = vol.clone()
    for a, b, c in rng.integers(1, N - 4, (opt.blobs, 3)).tolist():
        planted[a - 1:a + 4, b - 1:b + 4, c - 1:c + 4] = -1000.0       # detached: a shell of outside points ...
        planted[a:a + 3, b:b + 3, c:c + 3] = 1000.0                     # ... around 27 inside points (a later blob may cut an earlier one)
    clean_kernels(planted, f"field + {opt.blobs} blobs")
    del planted

# ---- the whole callers.extract_mesh, wall time ----------------------------------------------------------------------------------------
mod = S_.TextureEmbeddingPiGAN128SEMANTICDISENTANGLE(hidden_dim=256, z_geo_dim=8, z_app_dim=8, output_dim=22)
tsd = {k: torch.from_numpy(v) for k, v in sd.items()}
mod.spatial_embeddings = torch.nn.Parameter(tsd["spatial_embeddings"].clone())
mod.load_state_dict(tsd, strict=False)
mod.precision = "f16x3"
mod = mod.to(dev)
mod.device = torch.device(dev)
gen = types.SimpleNamespace(siren=mod, device=torch.device(dev))
meta = dict(truncated_frequencies_geo=fg, truncated_phase_shifts_geo=pg, truncated_frequencies_app=fa, truncated_phase_shifts_app=pa)
del vol
torch.cuda.empty_cache()
def wall(**kw):
    ts = []
    for i in range(4):          # the first call is the warm-up
        torch.cuda.synchronize(); t0 = time.perf_counter()
        m = callers.extract_mesh(gen, None, film=meta, voxel_resolution=N, cube_length=0.24, iso=iso, **kw)
        torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
    return m, ts[1:]
runs = [("defaults", {})] + [("keep='largest'", dict(keep="largest"))] * opt.keep_largest + \
    ([(f"keep={opt.min_component}", dict(keep=opt.min_component))] if opt.min_component is not None else []) + \
    ([(f"simplify={opt.simplify}", dict(simplify=opt.simplify))] if opt.simplify is not None else [])
for name, kw in runs:
    m, ts = wall(**kw)
    print(f"extract_mesh({name}): V={len(m['vertices'])} F={len(m['faces'])}{' components=%d' % m['components'] if 'components' in m else ''}; wall ms {ms(ts)}", flush=True)
    del m
