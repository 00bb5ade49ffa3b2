"""fenerf_volume_components / fenerf_volume_keep_components / fenerf_mesh_cluster_count / fenerf_mesh_cluster_emit
(fenerf_amd/csrc/fenerf_mesh_clean.hip) against their numpy restatement (fenerf_amd/mesh_emulation.py, itself held to independent statements
by tests/test_mesh_clean_cpu.py): labels and stats as integers, the filtered volume and the clustered vertices bit for bit, faces index for
index; then callers.extract_mesh(keep=, simplify=) and the flags of tools/extract_shapes.py end to end."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
from test_gpu_parity import DEV, N_, T
from test_mesh_clean_cpu import blob_case, serpentine, submesh, two_point_cases
from test_mesh_gpu import CUBE, RES, _generator, _smooth
from fenerf_amd import _lib, callers, imageio_lite, mesh_emulation as M, native

pytestmark = pytest.mark.gpu

FRAME = ((-0.11, 0.02, 0.3), (0.01, 0.02, 0.005))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _check_components(vol, iso):
    """labels and stats of the kernels == the emulation's; -> (labels, stats) as numpy"""
    labels, stats = native.volume_components(T(vol), iso)
    assert labels.dtype == torch.int32 and stats.dtype == torch.int64 and labels.is_cuda and labels.shape == vol.shape
    labels, stats = N_(labels), N_(stats)
    rl, rs = M.components(vol, iso)
    assert np.array_equal(labels, rl), f"{int((labels != rl).sum())} of {labels.size} labels differ"
    assert np.array_equal(stats, rs), (stats, rs)
    return labels, stats


def _check_filter(vol, iso, labels, keep):
    out, stats = native.filter_volume(T(vol), iso, keep)
    want = M.keep_components(vol, labels, keep)
    assert np.array_equal(_bits(N_(out)), _bits(want)), keep
    return N_(out)


def _check_cluster(v, f, origin, spacing, shape, factor):
    cv, cf = native.cluster_mesh(T(v), torch.as_tensor(f, device=DEV), origin, spacing, shape, factor)
    assert cv.dtype == torch.float32 and cf.dtype == torch.int32 and cv.is_cuda and cf.is_cuda
    rv, rf = M.cluster(v, f, origin, spacing, shape, factor)
    assert cv.shape == rv.shape and cf.shape == rf.shape, (cv.shape, rv.shape, cf.shape, rf.shape)
    assert np.array_equal(_bits(N_(cv)), _bits(rv)), f"{int((_bits(N_(cv)) != _bits(rv)).sum())} of {rv.size} coordinates differ in their bits"
    assert np.array_equal(N_(cf), rf)
    return N_(cv), N_(cf)


def test_every_inside_pattern_of_one_cell():
    rng = np.random.default_rng(0)
    for pattern in range(256):
        mag = rng.uniform(0.2, 1.0, 8)
        vol = np.empty((2, 2, 2), np.float32)
        for o in range(8):
            vol[o & 1, (o >> 1) & 1, o >> 2] = mag[o] if (pattern >> o) & 1 else -mag[o]
        labels, stats = _check_components(vol, 0.0)
        assert stats[0] == bin(pattern).count("1")
        _check_filter(vol, 0.0, labels, "largest")


def test_adjacency_is_the_fourteen_neighbourhood():
    n = 0
    for vol, d, adjacent in two_point_cases():
        labels, stats = _check_components(vol, 0.0)
        assert stats[1] == (1 if adjacent else 2), d
        n += adjacent
    assert n == 14


@functools.lru_cache(maxsize=None)
def _case(shape, field):
    if field == "random":
        vol, iso = np.random.default_rng(sum(shape)).normal(size=shape).astype(np.float32), 0.25
    else:
        # three separated lobes of the smooth field of the marching-tetrahedra test, cut by planes of low values
        vol, iso = _smooth(shape).copy(), 0.25
        vol[shape[0] // 3] = vol[:, shape[1] // 2] = -2
    vol.setflags(write=False)
    mesh = M.marching_tets(vol, iso, *FRAME, return_edges=True)
    return vol, iso, mesh


# 5 x 4 x 3, 3 x 2 x 70: less than one workgroup, odd axes, a long last axis.  65 x 33 x 31: 260 workgroups, not a multiple of anything.
# 70 x 64 x 64 = 286,720 points: 1,120 workgroups -- more partial results than the 1,024 threads of the stats workgroup take in one step, and
# (for the clustering of its mesh) more than 1,024 block counts: the running carry of the scans.
SHAPES = [((5, 4, 3), "random"), ((3, 2, 70), "random"), ((65, 33, 31), "random"), ((70, 64, 64), "smooth")]


@pytest.mark.parametrize("shape,field", SHAPES)
def test_components_and_keep_vs_emulation(shape, field):
    vol, iso, mesh = _case(shape, field)
    labels, stats = _check_components(vol, iso)
    assert stats[1] >= 2
    v, f = (N_(t) for t in native.mesh_from_volume(T(vol), iso, *FRAME))
    assert np.array_equal(_bits(v), _bits(mesh[0])) and np.array_equal(f, mesh[1])
    for keep in ("largest", 2, int(stats[3])):
        filtered = _check_filter(vol, iso, labels, keep)
        # through the unchanged marching tetrahedra: exactly the sub-mesh, bit for bit and in order
        kv, kf = (N_(t) for t in native.mesh_from_volume(T(filtered), iso, *FRAME))
        sv, sf = submesh(vol, iso, labels, filtered, (v, f, mesh[2]))
        assert np.array_equal(_bits(kv), _bits(sv)) and np.array_equal(kf, sf), keep
        assert 0 < len(kv) < len(v) or keep == 2
    print(f"[mesh clean] {shape} {field}: {stats[0]} inside points in {stats[1]} components, the largest {stats[3]} points at label {stats[2]}")


@pytest.mark.parametrize("shape,field", SHAPES)
def test_cluster_vs_emulation(shape, field):
    vol, iso, mesh = _case(shape, field)
    v, f = mesh[0], mesh[1]
    for factor in (2, 3):
        cv, cf = _check_cluster(v, f, *FRAME, shape, factor)
        assert len(cv) < len(v) and len(cf) < len(f)
        assert not len(cf) or ((cf[:, 0] != cf[:, 1]) & (cf[:, 1] != cf[:, 2]) & (cf[:, 0] != cf[:, 2])).all()
        assert np.array_equal(np.unique(cf), np.arange(len(cv)))
        print(f"[mesh clean] {shape} {field} factor {factor}: {len(v)} -> {len(cv)} vertices, {len(f)} -> {len(cf)} faces")
    cv, cf = _check_cluster(v, f, *FRAME, shape, max(shape))          # one cell: every face collapses
    assert cv.shape == (0, 3) and cf.shape == (0, 3)
    # empty input: nothing to launch, an empty result
    cv, cf = native.cluster_mesh(T(v), torch.zeros((0, 3), dtype=torch.int32, device=DEV), *FRAME, shape, 2)
    assert cv.shape == (0, 3) and cf.shape == (0, 3)
    cv, cf = native.cluster_mesh(torch.zeros((0, 3), device=DEV), torch.zeros((0, 3), dtype=torch.int32, device=DEV), *FRAME, shape, 2)
    assert cv.shape == (0, 3) and cf.shape == (0, 3)


def test_serpentine_is_one_component():
    vol = serpentine()
    labels, stats = _check_components(vol, 0.0)
    assert stats[1] == 1 and stats[0] == stats[3] > 450
    assert np.array_equal(_bits(_check_filter(vol, 0.0, labels, "largest")), _bits(vol))


def test_ties_and_degenerate_volumes():
    tie = np.full((2, 2, 9), -1, np.float32)
    tie[0, 0, 1:3] = tie[1, 1, 6:8] = 1
    labels, stats = _check_components(tie, 0.0)
    assert stats.tolist() == [4, 2, 1, 2]                               # equal sizes: the smaller label wins
    kept = _check_filter(tie, 0.0, labels, "largest")
    assert (kept[0, 0, 1:3] == 1).all() and np.isneginf(kept[1, 1, 6:8]).all()
    none = np.full((3, 4, 5), -1, np.float32)
    labels, stats = _check_components(none, 0.0)
    assert stats.tolist() == [0, 0, -1, 0] and (labels == -1).all()
    for keep in ("largest", 3):
        assert np.array_equal(_bits(_check_filter(none, 0.0, labels, keep)), _bits(none))
    full = np.full((3, 4, 5), 1, np.float32)
    labels, stats = _check_components(full, 0.0)
    assert stats.tolist() == [60, 1, 0, 60] and (labels == 0).all()
    assert np.array_equal(_bits(_check_filter(full, 0.0, labels, 60)), _bits(full))
    assert np.isneginf(_check_filter(full, 0.0, labels, 61)).all()
    # a wall of NaNs is outside and separates; NaN bits (payload included) are copied as they are
    nan = np.full((4, 5, 6), 1, np.float32)
    nan[:, 2, :] = np.nan
    nan.view(np.uint32)[0, 2, 0] = 0x7fc12345
    labels, stats = _check_components(nan, 0.0)
    assert stats.tolist() == [96, 2, 0, 48] and (labels[:, 2, :] == -1).all()
    out = _check_filter(nan, 0.0, labels, "largest")
    assert out.view(np.uint32)[0, 2, 0] == 0x7fc12345 and np.isneginf(out[:, 3:, :]).all() and (out[:, :2, :] == 1).all()


def test_filter_in_place_and_two_runs_give_identical_bytes():
    vol, iso, mesh = _case((65, 33, 31), "random")
    tv = T(vol)
    a, b = native.volume_components(tv, iso), native.volume_components(tv, iso)
    assert N_(a[0]).tobytes() == N_(b[0]).tobytes() and N_(a[1]).tobytes() == N_(b[1]).tobytes()
    fa, fb = native.filter_volume(tv, iso, 3)[0], native.filter_volume(tv, iso, 3)[0]
    assert N_(fa).tobytes() == N_(fb).tobytes()
    alias = tv.clone()
    out, _ = native.filter_volume(alias, iso, 3, out=alias)             # vol_out may be vol
    assert out.data_ptr() == alias.data_ptr() and N_(alias).tobytes() == N_(fa).tobytes()
    tvert, tf = T(mesh[0]), torch.as_tensor(mesh[1], device=DEV)
    ca, cb = native.cluster_mesh(tvert, tf, *FRAME, vol.shape, 2), native.cluster_mesh(tvert, tf, *FRAME, vol.shape, 2)
    assert ca[0].numel() and N_(ca[0]).tobytes() == N_(cb[0]).tobytes() and N_(ca[1]).tobytes() == N_(cb[1]).tobytes()


def test_c_abi_refusals():
    l = _lib.lib()
    shape = (4, 5, 6)
    vol = T(np.random.default_rng(3).normal(size=shape).astype(np.float32))
    p = lambda t: C.c_void_p(t.data_ptr())
    three = lambda *x: (C.c_float * 3)(*x)
    o3, s3 = three(0, 0, 0), three(1, 1, 1)
    ws = torch.empty(l.fenerf_volume_components_workspace_bytes(*shape), dtype=torch.uint8, device=DEV)
    labels = torch.empty(shape, dtype=torch.int32, device=DEV)
    stats = torch.zeros(4, dtype=torch.int64, device=DEV)
    out = torch.empty_like(vol)
    bad_shapes = ((1, 5, 6), (4, 1, 6), (4, 5, 1), (2048, 2048, 512))                 # an axis below 2; 2^31 points
    for sh in bad_shapes:
        assert l.fenerf_volume_components_workspace_bytes(*sh) == 0
        assert l.fenerf_volume_components(p(vol), *sh, 0.0, p(ws), p(labels), p(stats), None) == _lib.E_INVALID, sh
        assert l.fenerf_volume_keep_components(p(vol), p(labels), p(ws), *sh, _lib.KEEP_LARGEST, 1, p(out), None) == _lib.E_INVALID, sh
    for args in ((None, p(ws), p(labels), p(stats)), (p(vol), None, p(labels), p(stats)), (p(vol), p(ws), None, p(stats)), (p(vol), p(ws), p(labels), None)):
        assert l.fenerf_volume_components(args[0], *shape, 0.0, args[1], args[2], args[3], None) == _lib.E_INVALID
    assert "NULL" in l.fenerf_last_error().decode()
    _lib.check(l.fenerf_volume_components(p(vol), *shape, 0.0, p(ws), p(labels), p(stats), None))
    keep = lambda mode=_lib.KEEP_MIN_POINTS, mp=2, v=p(vol), lb=p(labels), w=p(ws), o=p(out): \
        l.fenerf_volume_keep_components(v, lb, w, *shape, mode, mp, o, None)
    assert keep(mode=2) == _lib.E_INVALID and keep(mode=-1) == _lib.E_INVALID
    assert keep(mp=0) == _lib.E_INVALID and keep(mp=-5) == _lib.E_INVALID and keep(mode=_lib.KEEP_LARGEST, mp=0) == _lib.E_INVALID
    assert keep(v=None) == _lib.E_INVALID and keep(lb=None) == _lib.E_INVALID and keep(w=None) == _lib.E_INVALID and keep(o=None) == _lib.E_INVALID
    _lib.check(keep())                                                                # the same stream still works: nothing was launched
    rl, rs = M.components(N_(vol), 0.0)
    assert np.array_equal(N_(labels), rl) and np.array_equal(N_(stats), rs)
    assert np.array_equal(_bits(N_(out)), _bits(M.keep_components(N_(vol), rl, 2)))

    # clustering
    rv, rf = M.marching_tets(N_(vol), 0.0)
    V, F = len(rv), len(rf)
    verts, faces = T(rv), torch.as_tensor(rf, device=DEV)
    cws = torch.empty(l.fenerf_mesh_cluster_workspace_bytes(V, F, *shape, 2), dtype=torch.uint8, device=DEV)
    counts = torch.zeros(3, dtype=torch.int64, device=DEV)
    count = lambda v=p(verts), nv=V, f=p(faces), nf=F, o=o3, s=s3, sh=shape, factor=2, w=p(cws), c=p(counts): \
        l.fenerf_mesh_cluster_count(v, nv, f, nf, o, s, *sh, factor, w, c, None)
    for sh in bad_shapes:
        assert l.fenerf_mesh_cluster_workspace_bytes(V, F, *sh, 2) == 0 and count(sh=sh) == _lib.E_INVALID, sh
    assert count(factor=1) == _lib.E_INVALID and count(factor=0) == _lib.E_INVALID and count(factor=-2) == _lib.E_INVALID
    assert count(nv=-1) == _lib.E_INVALID and count(nf=-1) == _lib.E_INVALID and count(nv=2 ** 31) == _lib.E_INVALID
    assert count(v=None) == _lib.E_INVALID and count(f=None) == _lib.E_INVALID and count(o=None) == _lib.E_INVALID and count(s=None) == _lib.E_INVALID
    assert count(w=None) == _lib.E_INVALID and count(c=None) == _lib.E_INVALID
    _lib.check(count())
    nv, nf, bad = (int(x) for x in counts.cpu())
    wv, wf = M.cluster(rv, rf, (0, 0, 0), (1, 1, 1), shape, 2)
    assert (nv, nf, bad) == (len(wv), len(wf), 0) and nv > 0 and nf > 0
    v_out = torch.empty((nv, 3), dtype=torch.float32, device=DEV)
    f_out = torch.empty((nf, 3), dtype=torch.int32, device=DEV)
    emit = lambda NV=nv, NF=nf, f=p(faces), o=o3, s=s3, sh=shape, factor=2, w=p(cws), pv=p(v_out), pf=p(f_out): \
        l.fenerf_mesh_cluster_emit(f, V, F, o, s, *sh, factor, w, NV, NF, pv, pf, None)
    for NV, NF in ((nv + 1, nf), (nv, nf - 1), (0, 0), (-1, nf), (nv, 2 ** 31)):     # not what the workspace holds
        assert emit(NV, NF) == _lib.E_INVALID, (NV, NF)
    assert emit(nv, nf - 1) == _lib.E_INVALID and "workspace holds" in l.fenerf_last_error().decode()
    assert emit(factor=1) == _lib.E_INVALID and emit(sh=(4, 1, 6)) == _lib.E_INVALID
    assert emit(f=None) == _lib.E_INVALID and emit(o=None) == _lib.E_INVALID and emit(s=None) == _lib.E_INVALID and emit(w=None) == _lib.E_INVALID
    assert emit(pv=None) == _lib.E_INVALID and emit(pf=None) == _lib.E_INVALID
    _lib.check(emit())
    assert np.array_equal(_bits(N_(v_out)), _bits(wv)) and np.array_equal(N_(f_out), wf)
    # a face index outside [0, V): found on the device, reported with the counts, refused by emit -- and never dereferenced
    broken = rf.copy()
    broken[1, 2], broken[5, 0] = V, -1
    tb = torch.as_tensor(broken, device=DEV)
    _lib.check(count(f=p(tb)))
    assert int(counts.cpu()[2]) == 2
    assert emit(f=p(tb)) == _lib.E_INVALID and "outside [0, V)" in l.fenerf_last_error().decode()
    with pytest.raises(_lib.FenerfError) as err:
        native.cluster_mesh(verts, tb, (0, 0, 0), (1, 1, 1), shape, 2)
    assert err.value.code == _lib.E_INVALID
    _lib.check(count())
    _lib.check(emit())                                                                # and the stream still works
    assert np.array_equal(_bits(N_(v_out)), _bits(wv)) and np.array_equal(N_(f_out), wf)
    with pytest.raises(ValueError):
        native.filter_volume(vol, 0.0, "biggest")


# ------------------------------------------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------------------------------------------
def test_extract_mesh_keep_and_simplify():
    gen, mod, spec, sd, film, meta = _generator()
    vol = callers.sample_generator_wth_frequencies_phase_shifts(gen, meta, voxel_resolution=RES, cube_length=CUBE)
    iso = float(np.median(vol))
    kw = dict(film=meta, voxel_resolution=RES, cube_length=CUBE, iso=iso)
    base = callers.extract_mesh(gen, None, **kw)
    same = callers.extract_mesh(gen, None, keep="all", simplify=None, **kw)
    assert sorted(base) == sorted(same) == ["faces", "label", "normal", "rgb", "vertices"]
    for k in base:
        assert base[k].dtype == same[k].dtype and base[k].tobytes() == same[k].tobytes(), k
    _, origin, size = callers.create_samples(RES, (0, 0, 0), CUBE, device=DEV)
    frame = ((origin[2], origin[1], origin[0]), (size,) * 3)
    full = M.marching_tets(vol, iso, *frame, return_edges=True)
    assert np.array_equal(_bits(base["vertices"]), _bits(full[0])) and np.array_equal(base["faces"], full[1])
    labels, stats = M.components(vol, iso)
    # keep: the sub-mesh of the unfiltered result, attributes of matching length
    for keep in ("largest", 2):
        mesh = callers.extract_mesh(gen, None, keep=keep, **kw)
        assert sorted(mesh) == ["components", "faces", "label", "normal", "rgb", "vertices"] and mesh["components"] == stats[1]
        sv, sf = submesh(vol, np.float32(iso), labels, M.keep_components(vol, labels, keep), full)
        V = len(mesh["vertices"])
        assert V > 0 and np.array_equal(_bits(mesh["vertices"]), _bits(sv)) and np.array_equal(mesh["faces"], sf)
        assert mesh["label"].shape == (V,) and mesh["rgb"].shape == (V, 3) and mesh["normal"].shape == (V, 3)
    # simplify: fewer vertices, the emulation's clustering of the full mesh, attributes evaluated at the vertices that survive
    mesh = callers.extract_mesh(gen, None, simplify=2, **kw)
    assert sorted(mesh) == ["faces", "label", "normal", "rgb", "vertices"]
    cv, cf = M.cluster(full[0], full[1], *frame, (RES,) * 3, 2)
    V, f = len(mesh["vertices"]), mesh["faces"]
    assert 0 < V < len(base["vertices"]) and np.array_equal(_bits(mesh["vertices"]), _bits(cv)) and np.array_equal(f, cf)
    assert ((f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])).all() and np.array_equal(np.unique(f), np.arange(V))
    assert mesh["label"].shape == (V,) and mesh["rgb"].shape == (V, 3) and mesh["normal"].shape == (V, 3)
    np.testing.assert_allclose(np.linalg.norm(mesh["normal"], axis=-1), 1, atol=1e-5)
    pad = (-V) % 32
    pts = np.concatenate([mesh["vertices"], np.repeat(mesh["vertices"][-1:], pad, 0)])[None]
    with torch.no_grad():
        rows = N_(mod.native(DEV).siren_forward(T(pts), None, film["freq_geo"], film["phase_geo"], film["freq_app"], film["phase_app"]))[0, :V]
    assert np.array_equal(mesh["label"], np.argmax(rows[:, :-4], axis=1))
    both = callers.extract_mesh(gen, None, keep="largest", simplify=3, attributes=("label",), **kw)
    assert sorted(both) == ["components", "faces", "label", "vertices"] and 0 < len(both["vertices"]) < V
    print(f"[mesh clean] extract_mesh {RES}^3: {stats[1]} components; {len(base['vertices'])} vertices -> {V} at simplify=2, {len(both['vertices'])} at largest + 3")
    for bad in (dict(keep="biggest"), dict(keep=0), dict(simplify=1), dict(simplify=2.5)):
        with pytest.raises(ValueError):
            callers.extract_mesh(gen, None, **bad, **kw)


def test_extract_shapes_tool_flags_write_a_clean_ply(tmp_path):
    ckpt = os.path.join(GOLDEN, "ref_generator_tiny.pth")
    gen = callers.load_generator(ckpt, DEV, use_ema=False)
    torch.manual_seed(3)
    z = torch.randn(1, callers._latent_dims(gen)[0], device=DEV)
    vol = callers.sample_generator(gen, z, cube_length=0.3, voxel_resolution=12)
    iso = float(np.median(vol))
    out = str(tmp_path / "shapes")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "extract_shapes.py"), ckpt, "--no_ema", "--seeds", "3", "--cube_size", "0.3",
                        "--voxel_resolution", "12", "--output_dir", out, "--mesh", "--iso", repr(iso), "--min_component", "2", "--simplify", "2"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "components before filtering" in r.stdout
    mesh = imageio_lite.read_ply(os.path.join(out, "3.ply"))
    frame = ((-0.15,) * 3, (0.3 / 11,) * 3)
    labels, _ = M.components(vol, np.float32(iso))
    rv, rf = M.marching_tets(M.keep_components(vol, labels, 2), np.float32(iso), *frame)
    cv, cf = M.cluster(rv, rf, *frame, (12, 12, 12), 2)
    V = len(cv)
    assert V > 0 and np.array_equal(_bits(mesh["vertices"]), _bits(cv)) and np.array_equal(mesh["faces"], cf)
    assert mesh["normal"].shape == (V, 3) and mesh["rgb"].shape == (V, 3) and mesh["label"].shape == (V,)
