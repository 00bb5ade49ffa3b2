"""Marching tetrahedra as include/fenerf.h states it, on its numpy restatement (fenerf_amd/mesh_emulation.py -- the yardstick the GPU tests
hold the kernels to), and the PLY writer / reader.  Nothing here touches the kernels."""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from fenerf_amd import imageio_lite, mesh_emulation as M

R0 = 0.7


def sphere_volume(n, centre=(0.0, 0.0, 0.0), r0=R0):
    """r0 - |x - centre| on the n^3 lattice of [-1, 1]^3 (fp32 values of an fp64 evaluation)"""
    g = np.linspace(-1, 1, n)
    x, y, z = np.meshgrid(g - centre[0], g - centre[1], g - centre[2], indexing="ij")
    return (r0 - np.sqrt(x * x + y * y + z * z)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def sphere_mesh(n):
    vol = sphere_volume(n)
    sp = 2.0 / (n - 1)
    verts, faces, edges = M.marching_tets(vol, 0.0, (-1, -1, -1), (sp, sp, sp), return_edges=True)
    for a in (vol, verts, faces) + edges:
        a.setflags(write=False)
    return vol, verts, faces, edges


def directed_edges(faces):
    f = np.asarray(faces, dtype=np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def unpaired_edges(faces):
    """directed edges whose reverse does not occur; asserts that no directed edge occurs twice"""
    e = directed_edges(faces)
    big = int(e.max()) + 1
    key, rkey = e[:, 0] * big + e[:, 1], e[:, 1] * big + e[:, 0]
    assert np.unique(key).size == key.size, "a directed edge occurs twice"
    return e[~np.isin(key, rkey)]


def signed_volume(verts, faces):
    p = verts.astype(np.float64)
    a, b, c = p[faces[:, 0]], p[faces[:, 1]], p[faces[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6)


@pytest.mark.parametrize("n", [17, 33])
def test_closed_sphere_is_a_closed_outward_manifold(n):
    vol, verts, faces, (pi, pk, t) = sphere_mesh(n)
    assert verts.dtype == np.float32 and faces.dtype == np.int32 and faces.min() == 0 and faces.max() == len(verts) - 1
    assert unpaired_edges(faces).size == 0                           # every directed edge once, its reverse once
    E = 3 * len(faces) // 2
    assert len(verts) - E + len(faces) == 2
    p = verts.astype(np.float64)
    a, b, c = p[faces[:, 0]], p[faces[:, 1]], p[faces[:, 2]]
    assert (np.einsum("ij,ij->i", np.cross(b - a, c - a), (a + b + c) / 3) > 0).all()      # the sphere's centre is the origin
    # every vertex on its lattice edge
    assert ((0 <= t) & (t <= 1)).all()
    sp = 2.0 / (n - 1)
    d = np.stack([pk & 1, (pk >> 1) & 1, (pk >> 2) & 1], -1)
    q = np.stack([pi // (n * n), (pi // n) % n, pi % n], -1)
    np.testing.assert_allclose(p, -1 + (q + t[:, None].astype(np.float64) * d) * sp, rtol=0, atol=4e-7)
    off = d == 0                                                      # the two (or one) coordinates an edge does not move along: the lattice's own
    lattice = (np.float32(-1) + q.astype(np.float32) * np.float32(sp)).astype(np.float32)
    assert np.array_equal(verts[off], lattice[off])
    # ascending (i, k) numbering
    assert (np.diff(pi * 8 + pk) > 0).all()


def test_sphere_volume_error_shrinks_with_resolution():
    exact = 4 / 3 * np.pi * R0 ** 3
    err = {n: abs(signed_volume(*sphere_mesh(n)[1:3]) - exact) for n in (17, 33, 65)}
    print(f"[mesh] |signed volume - 4/3 pi r^3| at 17^3 / 33^3 / 65^3: {err[17]:.4e} / {err[33]:.4e} / {err[65]:.4e}")
    assert err[17] > err[33] > err[65]
    assert err[33] <= 1.5 * 5.7030e-3          # measured 5.7029e-3 (a chordal surface lies inside the sphere: second order in the spacing)


def test_sphere_cut_by_the_volume_boundary_is_open_only_there():
    n = 17
    vol = sphere_volume(n, centre=(0.8, -0.75, 0.1))
    verts, faces, (pi, pk, _) = M.marching_tets(vol, 0.0, return_edges=True)       # unit spacing: coordinates are lattice coordinates
    open_e = unpaired_edges(faces)
    assert open_e.size and open_e.size < directed_edges(faces).size // 4
    a, b = verts[open_e[:, 0]], verts[open_e[:, 1]]
    on_face = ((a == 0) & (b == 0)) | ((a == n - 1) & (b == n - 1))                   # both ends on the same face of the volume
    assert on_face.any(-1).all()


def _tet_gradient(w, vals):
    """gradient of the affine function through the four (vertex, value) pairs of a tet"""
    A = np.array([np.subtract(w[v], w[0]) for v in (1, 2, 3)], dtype=np.float64)
    return np.linalg.solve(A, np.array([vals[v] - vals[0] for v in (1, 2, 3)], dtype=np.float64))


def test_all_256_sign_patterns_of_one_cell():
    """Face count per tet from the sign pattern alone; winding by brute force: inside a tet the interpolated field is affine and every face lies
    in its iso-plane, so the face normal must point down the field's gradient."""
    rng = np.random.default_rng(0)
    for pattern in range(256):
        mag = rng.uniform(0.2, 1.0, 8)
        vol = np.empty((2, 2, 2), np.float32)
        for o in range(8):                                      # corner o: bit j = offset along axis j
            vol[o & 1, (o >> 1) & 1, o >> 2] = mag[o] if (pattern >> o) & 1 else -mag[o]
        verts, faces = M.marching_tets(vol, 0.0)
        mask, nf = M.classify(vol, 0.0)
        assert len(verts) == sum(bin(int(m)).count("1") for m in mask)
        per_tet = []
        for perm in M.PERMS:
            nin = sum(int(vol[w] >= 0) for w in M.tet_vertices(perm))
            per_tet.append({0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[nin])
        assert len(faces) == sum(per_tet) == int(nf[0])
        p = verts.astype(np.float64)
        at = 0
        for perm, cnt in zip(M.PERMS, per_tet):
            w = M.tet_vertices(perm)
            grad = _tet_gradient(w, [float(vol[x]) for x in w]) if cnt else None
            for f in faces[at:at + cnt]:
                a, b, c = p[f[0]], p[f[1]], p[f[2]]
                assert len(set(f.tolist())) == 3
                for x in (a, b, c):                             # the face belongs to this tet: its corners lie in the tet's closure
                    lam = np.linalg.solve(np.array([np.subtract(w[v], w[0]) for v in (1, 2, 3)], dtype=np.float64).T, x - np.array(w[0]))
                    assert (lam >= -1e-6).all() and lam.sum() <= 1 + 1e-6
                assert np.dot(np.cross(b - a, c - a), grad) < 0, (pattern, perm)
            at += cnt


def test_quads_split_along_the_diagonal_through_the_smallest_vertex_number():
    vol = sphere_mesh(17)[0]
    _, faces = sphere_mesh(17)[1:3]
    _, nf = M.classify(vol, 0.0)
    assert int(nf.sum()) == len(faces) and nf.max() <= 12
    # faces are grouped by cell in cell order and by tet inside a cell; a tet with two inside vertices holds a quad
    starts = np.concatenate([[0], np.cumsum(nf.astype(np.int64))])
    quads = 0
    for j in np.nonzero(nf)[0][:400]:
        c = np.array([j // 256, (j // 16) % 16, j % 16])
        at = starts[j]
        for perm in M.PERMS:
            nin = sum(int(vol[tuple(c + w)] >= 0) for w in M.tet_vertices(perm))
            if nin == 2:
                f, g = faces[at], faces[at + 1]
                assert len({*f.tolist(), *g.tolist()}) == 4 and f[0] == g[0] == min(f.min(), g.min()) and f[2] == g[1]
                quads += 1
            at += {0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[nin]
        assert at == starts[j + 1]
    assert quads > 50


def test_values_equal_to_iso_are_inside_and_keep_their_zero_area_faces():
    g = np.arange(-4, 5)
    x, y, z = np.meshgrid(g, g, g, indexing="ij")
    vol = (9 - (x * x + y * y + z * z)).astype(np.float32)          # exact zeros at (+-3, 0, 0), (+-2, +-2, +-1), ...
    assert (vol == 0).sum() >= 30
    verts, faces, (pi, pk, t) = M.marching_tets(vol, 0.0, return_edges=True)
    mask, nf = M.classify(vol, 0.0)
    assert len(faces) == int(nf.sum()) and len(verts) == int(M._POP8[mask].sum())
    assert (t == 0).any() and ((0 <= t) & (t <= 1)).all() and np.isfinite(verts).all()
    # a tie is inside: the mesh is that of the field lifted by less than any gap between its values, vertex for vertex, face for face
    v2, f2 = M.marching_tets(vol + np.float32(0.25), 0.0)
    assert np.array_equal(faces, f2) and len(v2) == len(verts)
    assert unpaired_edges(faces).size == 0 and len(verts) - 3 * len(faces) // 2 + len(faces) == 2
    p = verts.astype(np.float64)
    area = np.linalg.norm(np.cross(p[faces[:, 1]] - p[faces[:, 0]], p[faces[:, 2]] - p[faces[:, 0]]), axis=1)
    assert (area == 0).any() and (area > 0).any()


@pytest.mark.parametrize("fill", [-1.0, 1.0, np.nan])
def test_volumes_without_a_crossing_give_empty_meshes(fill):
    verts, faces = M.marching_tets(np.full((3, 4, 5), fill, np.float32), 0.0)
    assert verts.shape == (0, 3) and verts.dtype == np.float32 and faces.shape == (0, 3) and faces.dtype == np.int32


def test_non_finite_values_touch_only_their_own_vertices():
    rng = np.random.default_rng(5)
    vol = rng.normal(size=(9, 9, 9)).astype(np.float32)
    planted = {(2, 3, 4): np.nan, (5, 5, 5): np.inf, (6, 2, 7): -np.inf}
    clean = vol.copy()
    for q, v in planted.items():
        vol[q] = v
        clean[q] = 1.0 if v == np.inf else -1.0                      # NaN and -Inf are not inside, +Inf is
    verts, faces, (pi, pk, _) = M.marching_tets(vol, 0.0, return_edges=True)
    v_ref, f_ref = M.marching_tets(clean, 0.0)
    assert np.array_equal(faces, f_ref) and verts.shape == v_ref.shape
    lin = {(a * 9 + b) * 9 + c for a, b, c in planted}
    qi = pi + (pk & 1) * 81 + ((pk >> 1) & 1) * 9 + (pk >> 2)
    touched = np.array([int(a) in lin or int(b) in lin for a, b in zip(pi, qi)])
    bad = ~np.isfinite(verts).all(-1)
    assert bad.any() and not (bad & ~touched).any()
    assert np.array_equal(verts[~touched], v_ref[~touched])


def test_ply_round_trip_and_exact_header(tmp_path):
    rng = np.random.default_rng(1)
    v = rng.normal(size=(5, 3)).astype(np.float32)
    f = np.array([[0, 1, 2], [2, 3, 4], [4, 0, 1]], np.int32)
    nrm = rng.normal(size=(5, 3)).astype(np.float32)
    rgb = rng.integers(0, 256, (5, 3)).astype(np.uint8)
    lab = rng.integers(0, 18, 5).astype(np.uint8)
    path = str(tmp_path / "m.ply")
    imageio_lite.write_ply(path, v, f, normal=nrm, rgb=rgb, label=lab)
    raw = open(path, "rb").read()
    header = (b"ply\nformat binary_little_endian 1.0\ncomment fenerf_amd.imageio_lite.write_ply\nelement vertex 5\n"
              b"property float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\nproperty float nz\n"
              b"property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar label\n"
              b"element face 3\nproperty list uchar int vertex_indices\nend_header\n")
    assert raw.startswith(header) and len(raw) == len(header) + 5 * (24 + 4) + 3 * 13
    assert np.array_equal(np.frombuffer(raw, "<f4", 3, len(header)), v[0]) and raw[len(header) + 5 * 28] == 3
    back = imageio_lite.read_ply(path)
    for k, ref in dict(vertices=v, faces=f, normal=nrm, rgb=rgb, label=lab).items():
        assert back[k].dtype == ref.dtype and np.array_equal(back[k], ref), k
    # positions and faces alone; an empty mesh
    imageio_lite.write_ply(path, v, f)
    back = imageio_lite.read_ply(path)
    assert sorted(back) == ["faces", "vertices"] and np.array_equal(back["vertices"], v) and np.array_equal(back["faces"], f)
    assert b"property float nx" not in open(path, "rb").read()
    imageio_lite.write_ply(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), label=np.zeros(0, np.uint8))
    back = imageio_lite.read_ply(path)
    assert back["vertices"].shape == (0, 3) and back["faces"].shape == (0, 3) and back["label"].shape == (0,)
    open(path, "wb").write(b"ply\nformat ascii 1.0\nend_header\n")
    with pytest.raises(ValueError):
        imageio_lite.read_ply(path)


def test_mesh_entry_points_are_declared_exported_and_reachable():
    from fenerf_amd import _lib, callers, native
    hdr = open(os.path.join(ROOT, "include", "fenerf.h")).read()
    for name in ("fenerf_mesh_workspace_bytes", "fenerf_mesh_count", "fenerf_mesh_emit"):
        assert name + "(" in hdr and name in _lib.EXPORTS
    assert "#define FENERF_ABI_VERSION 2" in hdr
    assert callable(native.mesh_from_volume) and callable(callers.extract_mesh)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import extract_shapes
    finally:
        sys.path.pop(0)
    s = extract_shapes.build_parser().parse_args(["g.pth"])
    assert (s.mesh, s.iso) == (False, 10.0)
    s = extract_shapes.build_parser().parse_args(["g.pth", "--mesh", "--iso", "2.5"])
    assert (s.mesh, s.iso) == (True, 2.5)
    # invalid lattices need no device: refused before anything is touched
    l = _lib.lib()
    assert l.fenerf_mesh_workspace_bytes(1, 4, 4) == 0 and l.fenerf_mesh_workspace_bytes(2048, 2048, 512) == 0
    n = 5 * 4 * 3
    assert n * 5 + 2 * 3 * 4 <= l.fenerf_mesh_workspace_bytes(5, 4, 3) <= n * 5 + 24 + 8 * 256       # ~5 bytes per point + 1 per cell, 256-aligned parts
