"""numpy restatement of fenerf_mesh_count / fenerf_mesh_emit (fenerf_amd/csrc/fenerf_mesh.hip, include/fenerf.h): marching tetrahedra on the
Kuhn decomposition of a lattice, in the kernels' integer and float32 arithmetic step by step, so that the library's vertices can be
checked bit for bit and its faces index for index on the CPU side.

Conventions (include/fenerf.h states the same):
  - vol [n0][n1][n2] float32; point p = (a, b, c) has linear index i = (a * n1 + b) * n2 + c; inside(p) := vol[p] >= iso (a NaN is not).
  - a cell is a point c with c + (1, 1, 1) in the lattice; six tets per cell, one per axis permutation PERMS[t]: vertices
    c, c + e_pi0, c + e_pi0 + e_pi1, c + (1, 1, 1).
  - every tet edge is owned by its lower endpoint p as edge k = 1 .. 7 of direction d_k = (k & 1, (k >> 1) & 1, (k >> 2) & 1); an owned edge
    whose endpoints differ in `inside` carries one vertex; vertices are numbered in ascending (i, k).
  - position: t = (iso - vol[p]) / (vol[q] - vol[p]); coordinate j = origin[j] + (p_j + t * d_kj) * spacing[j], every operation fp32.
  - a tet emits 0, 1 or 2 triangles over its crossing edges; a quad is split along the diagonal through its smallest vertex number;
    (v1 - v0) x (v2 - v0) points to the not-inside side; faces are ordered by cell, tet, triangle.

Further down: components / keep_components / cluster restate the mesh-cleaning calls (fenerf_amd/csrc/fenerf_mesh_clean.hip) the same way."""
import numpy as np

PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))


def tet_vertices(perm):
    """the four vertex offsets of the Kuhn tet of an axis permutation, along its lattice path"""
    w = [[0, 0, 0]]
    for axis in perm:
        nxt = list(w[-1])
        nxt[axis] = 1
        w.append(nxt)
    return (tuple(w[0]), tuple(w[1]), tuple(w[2]), (1, 1, 1))


def _cross(u, v):
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


def tet_case(perm, s):
    """Crossing edges of one tet whose vertex v is inside iff bit v of s is set, as (corner offset of the lower endpoint, k) pairs:
    () for no face, three edges for one triangle, four edges in cyclic order for a quad -- wound so that the normal of the first three points
    to the not-inside side.  The winding comes from integer geometry alone: the edge midpoints (doubled, to stay integral) stand in for the
    vertices, and the direction from the inside vertices' centroid to the other vertices' centroid is the reference."""
    w = tet_vertices(perm)
    ins = [v for v in range(4) if (s >> v) & 1]
    out = [v for v in range(4) if not (s >> v) & 1]
    if not ins or not out:
        return ()
    if len(ins) == 1:
        pairs = [(ins[0], b) for b in out]
    elif len(out) == 1:
        pairs = [(out[0], b) for b in ins]
    else:
        pairs = [(ins[0], out[0]), (ins[0], out[1]), (ins[1], out[1]), (ins[1], out[0])]
    mid = [tuple(w[a][x] + w[b][x] for x in range(3)) for a, b in pairs]
    nrm = _cross(tuple(mid[1][x] - mid[0][x] for x in range(3)), tuple(mid[2][x] - mid[0][x] for x in range(3)))
    ref = tuple(len(ins) * sum(w[v][x] for v in out) - len(out) * sum(w[v][x] for v in ins) for x in range(3))
    dot = sum(nrm[x] * ref[x] for x in range(3))
    assert dot != 0
    if dot < 0:
        pairs = [pairs[0]] + pairs[:0:-1]
    edges = []
    for a, b in pairs:
        lo, hi = w[min(a, b)], w[max(a, b)]
        d = tuple(hi[x] - lo[x] for x in range(3))
        edges.append((lo, d[0] | d[1] << 1 | d[2] << 2))
    return tuple(edges)


TABLE = tuple(tuple(tet_case(perm, s) for s in range(16)) for perm in PERMS)
_POP8 = np.array([bin(v).count("1") for v in range(256)], dtype=np.int64)


def classify(vol, iso):
    """-> (mask uint8 [n]: bit k - 1 set when owned edge k of the point crosses, faces uint8 [cells]: 0 .. 12 per cell in cell order)"""
    vol = np.asarray(vol, dtype=np.float32)
    n0, n1, n2 = vol.shape
    with np.errstate(invalid="ignore"):
        inside = vol >= np.float32(iso)
    mask = np.zeros(vol.shape, dtype=np.uint8)
    for k in range(1, 8):
        d = (k & 1, (k >> 1) & 1, (k >> 2) & 1)
        lo = inside[:n0 - d[0], :n1 - d[1], :n2 - d[2]]
        hi = inside[d[0]:, d[1]:, d[2]:]
        mask[:n0 - d[0], :n1 - d[1], :n2 - d[2]] |= ((lo != hi).astype(np.uint8) << (k - 1)).astype(np.uint8)
    faces = np.zeros((n0 - 1, n1 - 1, n2 - 1), dtype=np.uint8)
    for perm in PERMS:
        nin = np.zeros(faces.shape, dtype=np.int64)
        for o in tet_vertices(perm):
            nin += inside[o[0]:n0 - 1 + o[0], o[1]:n1 - 1 + o[1], o[2]:n2 - 1 + o[2]]
        faces += np.where(nin == 2, 2, np.where((nin == 1) | (nin == 3), 1, 0)).astype(np.uint8)
    return mask.reshape(-1), faces.reshape(-1)


def marching_tets(vol, iso, origin=(0, 0, 0), spacing=(1, 1, 1), return_edges=False):
    """-> (vertices [V,3] float32, faces [F,3] int32), what fenerf_mesh_count + fenerf_mesh_emit write.
    return_edges: also (owner point index [V] int64, edge k [V], t [V] float32) of every vertex."""
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    n0, n1, n2 = vol.shape
    assert min(vol.shape) >= 2
    iso = np.float32(iso)
    origin, spacing = np.asarray(origin, dtype=np.float32), np.asarray(spacing, dtype=np.float32)
    flat = vol.reshape(-1)
    mask, _ = classify(vol, iso)
    cross = ((mask[:, None] >> np.arange(7, dtype=np.uint8)[None, :]) & 1).astype(bool)          # [n, 7], column k - 1
    prefix = np.cumsum(_POP8[mask]) - _POP8[mask]                                                 # exclusive, int64
    pi, pk = np.nonzero(cross)                                                                    # ascending (i, k)
    pk = pk + 1
    d = np.stack([pk & 1, (pk >> 1) & 1, (pk >> 2) & 1], -1)
    p = np.stack([pi // (n1 * n2), (pi // n2) % n1, pi % n2], -1)
    qi = pi + d[:, 0] * (n1 * n2) + d[:, 1] * n2 + d[:, 2]
    with np.errstate(all="ignore"):
        vp, vq = flat[pi], flat[qi]
        t = ((iso - vp) / (vq - vp)).astype(np.float32)
        verts = origin[None, :] + (p.astype(np.float32) + t[:, None] * d.astype(np.float32)) * spacing[None, :]
    verts = verts.astype(np.float32).reshape(-1, 3)

    def number(i, k):       # the kernels' lookup: prefix of the owner + the crossing edges below k
        return prefix[i] + _POP8[mask[i] & ((1 << (k - 1)) - 1)]

    with np.errstate(invalid="ignore"):
        inside = (vol >= iso)
    ca, cb, cc = np.meshgrid(np.arange(n0 - 1), np.arange(n1 - 1), np.arange(n2 - 1), indexing="ij")
    ci = ((ca * n1 + cb) * n2 + cc).reshape(-1)                                                   # linear index of every cell's corner c
    cell = np.arange(ci.size)
    tris, keys = [], []
    for ti, perm in enumerate(PERMS):
        s = np.zeros(ci.size, dtype=np.int64)
        for v, o in enumerate(tet_vertices(perm)):
            s |= inside[o[0]:n0 - 1 + o[0], o[1]:n1 - 1 + o[1], o[2]:n2 - 1 + o[2]].reshape(-1).astype(np.int64) << v
        for case in range(1, 15):
            sel = np.nonzero(s == case)[0]
            if not sel.size:
                continue
            vn = np.stack([number(ci[sel] + (o[0] * n1 + o[1]) * n2 + o[2], k) for o, k in TABLE[ti][case]], -1)
            if vn.shape[1] == 3:
                tris.append(vn)
                keys.append(np.stack([cell[sel], np.full(sel.size, ti), np.zeros(sel.size, dtype=np.int64)], -1))
            else:
                m = np.argmin(vn, axis=1)
                r = np.arange(sel.size)
                for j, (x, y) in enumerate(((1, 2), (2, 3))):
                    tris.append(np.stack([vn[r, m], vn[r, (m + x) % 4], vn[r, (m + y) % 4]], -1))
                    keys.append(np.stack([cell[sel], np.full(sel.size, ti), np.full(sel.size, j)], -1))
    if tris:
        tris, keys = np.concatenate(tris), np.concatenate(keys)
        order = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
        faces = tris[order].astype(np.int32)
    else:
        faces = np.zeros((0, 3), dtype=np.int32)
    if return_edges:
        return verts, faces, (pi, pk, t)
    return verts, faces


def canonical_faces(faces):
    """every triangle rotated to put its smallest index first, rows sorted: equal for two meshes with the same oriented triangles"""
    f = np.asarray(faces).reshape(-1, 3)
    if not f.shape[0]:
        return f
    m = np.argmin(f, axis=1)
    r = np.arange(f.shape[0])
    f = np.stack([f[r, m], f[r, (m + 1) % 3], f[r, (m + 2) % 3]], -1)
    return f[np.lexsort((f[:, 2], f[:, 1], f[:, 0]))]


# ---- mesh cleaning (fenerf_amd/csrc/fenerf_mesh_clean.hip): components of the inside set, vertex clustering --------------------------------
KEEP_LARGEST = "largest"


def components(vol, iso):
    """-> (labels int32 [n0,n1,n2], stats int64 [4]), what fenerf_volume_components writes.  Two inside points are adjacent when they differ
    by +-d_k, k = 1 .. 7 (the Kuhn tetrahedra's edges: 14 neighbours); a component's label is its smallest linear index, -1 outside.
    stats = inside points, components, label of the largest component (a tie: the smaller label; -1 with no inside point), its point count.
    The kernels reach the labels by union-find with atomicMin; the result does not depend on the route, so this walks another one: every
    inside point takes the smallest label among itself and its neighbours, then jumps to its label's label, until nothing changes."""
    vol = np.asarray(vol, dtype=np.float32)
    n0, n1, n2 = vol.shape
    with np.errstate(invalid="ignore"):
        inside = vol >= np.float32(iso)
    n = vol.size
    big = np.int64(n)
    lab = np.where(inside, np.arange(n, dtype=np.int64).reshape(vol.shape), big)
    while True:
        new = lab.copy()
        for k in range(1, 8):
            d = (k & 1, (k >> 1) & 1, (k >> 2) & 1)
            lo = (slice(0, n0 - d[0]), slice(0, n1 - d[1]), slice(0, n2 - d[2]))
            hi = (slice(d[0], n0), slice(d[1], n1), slice(d[2], n2))
            both = inside[lo] & inside[hi]
            m = np.minimum(new[lo], new[hi])
            new[lo] = np.where(both, m, new[lo])
            new[hi] = np.where(both, np.minimum(m, new[hi]), new[hi])       # lo and hi overlap: never raise what the line above lowered
        flat = new.reshape(-1)
        ins = inside.reshape(-1)
        flat[ins] = flat[flat[ins]]              # a label is the index of a point of the same component
        if np.array_equal(new, lab):
            break
        lab = new
    labels = np.where(inside, lab, -1).astype(np.int32)
    counts = component_counts(labels)
    roots = np.nonzero(counts)[0]
    stats = np.array([int(inside.sum()), roots.size, -1, 0], dtype=np.int64)
    if roots.size:
        best = roots[np.argmax(counts[roots])]      # argmax takes the first of equal counts: the smaller label
        stats[2], stats[3] = best, counts[best]
    return labels, stats


def component_counts(labels):
    """int64 [n]: the point count of every component at its label's own index (what the kernels keep in the workspace), 0 elsewhere"""
    flat = np.asarray(labels).reshape(-1)
    return np.bincount(flat[flat >= 0], minlength=flat.size).astype(np.int64)


def keep_components(vol, labels, keep):
    """-> vol with every inside point of a dropped component replaced by -inf, everything else bit for bit (fenerf_volume_keep_components).
    keep = "largest" (by point count, a tie to the smaller label), or an int: every component of at least that many points stays."""
    vol = np.asarray(vol, dtype=np.float32)
    labels = np.asarray(labels).reshape(vol.shape)
    counts = component_counts(labels)
    if keep == KEEP_LARGEST:
        kept = np.zeros(counts.size, dtype=bool)
        if counts.any():
            kept[np.argmax(counts)] = True
    else:
        if int(keep) < 1:
            raise ValueError("keep_components: min_points < 1")
        kept = counts >= int(keep)
    out = vol.copy()
    drop = (labels >= 0) & ~kept[np.maximum(labels, 0)]
    out[drop] = -np.inf
    return out


def cluster(vertices, faces, origin, spacing, shape, factor):
    """-> (vertices [V',3] float32, faces [F',3] int32), what fenerf_mesh_cluster_count + fenerf_mesh_cluster_emit write.  Per vertex and axis:
    u = (x - origin) / spacing in fp32, cell = clamp(floor(u / factor), 0, ceil((n - 1) / factor) - 1), cluster id = linear index of the
    cell; the representative is the members' mean in 2^-16 lattice units summed as int64; new vertices in ascending cluster id over the
    clusters a surviving face references; a face with two equal new indices is dropped, the others keep order and winding; duplicate faces
    are not searched for.  A face index outside [0, V) raises ValueError (the library: FENERF_E_INVALID)."""
    v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    factor = int(factor)
    if factor < 2:
        raise ValueError("cluster: factor < 2")
    origin, spacing = np.asarray(origin, dtype=np.float32), np.asarray(spacing, dtype=np.float32)
    m = np.array([(int(n) - 1 + factor - 1) // factor for n in shape], dtype=np.int64)
    V = v.shape[0]
    if ((f < 0) | (f >= V)).any():
        raise ValueError("cluster: a face index outside [0, V)")
    empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    if not f.shape[0]:
        return empty
    with np.errstate(all="ignore"):
        u = ((v - origin[None, :]).astype(np.float32) / spacing[None, :]).astype(np.float32)
        fl = np.floor((u / np.float32(factor)).astype(np.float32))
        top = (m - 1).astype(np.float32)[None, :]
        cell = np.where(fl >= top, top, np.where(fl > 0, fl, np.float32(0))).astype(np.int64)      # a NaN falls into cell 0
        qd = u.astype(np.float64) * 65536.0
        ok = np.abs(qd) < 2.0 ** 62
        q = np.where(ok, np.rint(np.where(ok, qd, 0.0)), 0.0).astype(np.int64)
    cid = (cell[:, 0] * m[1] + cell[:, 1]) * m[2] + cell[:, 2]
    ncl = int(m.prod())
    sums = np.zeros((ncl, 3), dtype=np.int64)
    np.add.at(sums, cid, q)
    members = np.bincount(cid, minlength=ncl).astype(np.int64)
    fc = cid[f]                                                                                     # [F, 3] cluster ids
    keep = (fc[:, 0] != fc[:, 1]) & (fc[:, 1] != fc[:, 2]) & (fc[:, 0] != fc[:, 2])
    used = np.zeros(ncl, dtype=bool)
    used[fc[keep].reshape(-1)] = True
    newid = np.cumsum(used) - 1
    ids = np.nonzero(used)[0]
    mean = sums[ids].astype(np.float64) / (members[ids].astype(np.float64) * 65536.0)[:, None]
    v_out = (origin.astype(np.float64)[None, :] + mean * spacing.astype(np.float64)[None, :]).astype(np.float32)
    f_out = newid[fc[keep]].astype(np.int32)
    return v_out.reshape(-1, 3), f_out.reshape(-1, 3)
