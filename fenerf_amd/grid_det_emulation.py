"""numpy restatement of fenerf_grid_backward_det (fenerf_amd/csrc/fenerf_grid_det.hip, include/fenerf.h): the deterministic gradient wrt the
feature grid, in the kernel's float32 / float64 / int64 arithmetic step by step, so that the library's result can be checked bit for bit
on the CPU side.  Also the fp64 transpose of sample_from_3dgrid (siren.py:314-330) it approximates."""
import numpy as np

BOX_SCALE = np.float32(2 / 0.24)      # UniformBoxWarp(0.24) as the model descriptor stores it (fenerf_amd/_lib.py make_desc)


def corners(points, grid_shape, box_scale=BOX_SCALE):
    """-> per corner c (z-major: cz = c >> 2, cy = (c >> 1) & 1, cx = c & 1): (in-bounds mask [rows], voxel index [rows], fp32 weight
    wx * wy * wz [rows]) -- grid_backward_kernel's float32 arithmetic"""
    D, Hh, W = grid_shape
    p = np.asarray(points, dtype=np.float32)
    one, two = np.float32(1), np.float32(2)
    with np.errstate(invalid="ignore", over="ignore"):
        q = p * np.float32(box_scale)
        ix = ((q[:, 0] + one) / two) * np.float32(W - 1)
        iy = ((q[:, 1] + one) / two) * np.float32(Hh - 1)
        iz = ((q[:, 2] + one) / two) * np.float32(D - 1)
        x0, y0, z0 = np.floor(ix), np.floor(iy), np.floor(iz)
        out = []
        for c in range(8):
            cz, cy, cx = c >> 2, (c >> 1) & 1, c & 1
            xi, yi, zi = x0 + np.float32(cx), y0 + np.float32(cy), z0 + np.float32(cz)
            wx = (ix - x0) if cx else (x0 + one - ix)
            wy = (iy - y0) if cy else (y0 + one - iy)
            wz = (iz - z0) if cz else (z0 + one - iz)
            ok = (xi >= 0) & (xi <= np.float32(W - 1)) & (yi >= 0) & (yi <= np.float32(Hh - 1)) & (zi >= 0) & (zi <= np.float32(D - 1))
            vox = np.zeros(p.shape[0], dtype=np.int64)
            vox[ok] = (zi[ok].astype(np.int64) * Hh + yi[ok].astype(np.int64)) * W + xi[ok].astype(np.int64)
            out.append((ok, vox, (wx * wy * wz).astype(np.float32)))
    return out


def shift(d_e, dense_rows):
    """k of the scale 2^k: 62 - e - h, max |finite d_e| < 2^e (frexp; 0 for an all-zero input), h = ceil(log2(dense_rows))"""
    a = np.abs(np.asarray(d_e, dtype=np.float32))
    a = a[np.isfinite(a)]
    m = np.float32(a.max()) if a.size else np.float32(0)
    e = int(np.frexp(m)[1])
    h = 0
    while (1 << h) < int(dense_rows):
        h += 1
    return 62 - e - h


def grid_backward_det(points, d_e, grid_shape, dense_rows, box_scale=BOX_SCALE):
    """-> channels-last gradient grid [D,H,W,32] float32, bit for bit what fenerf_grid_backward_det writes"""
    D, Hh, W = grid_shape
    d_e = np.asarray(d_e, dtype=np.float32).reshape(-1, 32)
    k = shift(d_e, dense_rows)
    scale = np.float64(2.0) ** k
    acc = np.zeros((D * Hh * W, 32), dtype=np.int64)
    fin = np.isfinite(d_e)
    use = fin & (d_e != 0)
    cs = corners(points, grid_shape, box_scale)
    rows, ch = np.nonzero(use)
    g = d_e[rows, ch]
    for ok, vox, w in cs:
        sel = ok[rows]
        v = (g[sel] * w[rows[sel]]).astype(np.float32)                  # fp32 product, like the kernel
        q = np.rint(v.astype(np.float64) * scale).astype(np.int64)
        np.add.at(acc, (vox[rows[sel]], ch[sel]), q)
    out = (acc.astype(np.float64) * (np.float64(2.0) ** -k)).astype(np.float32)
    bad_r, bad_c = np.nonzero(~fin)
    for ok, vox, _ in cs:
        sel = ok[bad_r]
        out[vox[bad_r[sel]], bad_c[sel]] = np.nan
    return out.reshape(D, Hh, W, 32)


def grid_backward_f64(points, d_e, grid_shape, box_scale=BOX_SCALE):
    """the same transpose summed in float64: np.add.at of the fp32 contributions g * (wx * wy * wz) (what both routes multiply; finite values
    only) -> [D,H,W,32] float64.  grid_backward_det differs from it by the rounding of each contribution to the int64 grid (resolution)
    and the final rounding to fp32."""
    D, Hh, W = grid_shape
    d_e = np.asarray(d_e, dtype=np.float32).reshape(-1, 32)
    acc = np.zeros((D * Hh * W, 32), dtype=np.float64)
    d_e = np.where(np.isfinite(d_e), d_e, np.float32(0))
    for ok, vox, w in corners(points, grid_shape, box_scale):
        r = np.nonzero(ok)[0]
        np.add.at(acc, vox[r], (d_e[r] * w[r, None]).astype(np.float32).astype(np.float64))
    return acc.reshape(D, Hh, W, 32)


def resolution(d_e, dense_rows):
    """the bound per contribution of the rounding to integers: 2^-(k+1) (half a unit of the int64 grid), k = shift(d_e, dense_rows)"""
    return 2.0 ** -(shift(d_e, dense_rows) + 1)
