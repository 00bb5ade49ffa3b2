"""numpy restatement of the free-camera kernels (csrc/fenerf_camera.hip, include/fenerf.h fenerf_camera_rays / fenerf_camera_grads).

`camera_rays` states camera_rays_kernel operation for operation: with dtype=np.float32 every product, sum, quotient and square root is
rounded on its own, as the kernel rounds them, and the result is the kernel's bits; with dtype=np.float64 the same statements are the
definition the kernel is held to.  `camera_grad_terms` gives, in fp64, the 17 per-ray terms whose sums over the rays of an image
fenerf_camera_grads returns -- the tests bound the kernel's sums by the sum of their magnitudes.

Test infrastructure and documentation of the arithmetic; the render path does not import it."""
import numpy as np


def linspace(start, end, steps, dtype=np.float32, fused=False):
    """torch.linspace's kernel: step = (end - start) / (steps - 1); i < steps // 2 ? start + step * i : end - step * (steps - 1 - i).
    fused: the product and the sum as one fused multiply-add (formed in fp64 -- the product of two fp32 values is exact there -- and
    rounded once): the sample depths.  Unfused: the pixel grid."""
    dt = np.dtype(dtype).type
    start, end = dt(start), dt(end)
    if steps == 1:
        return np.array([start], dtype=dt)
    step = dt(dt(end - start) / dt(steps - 1))
    i = np.arange(steps)
    wide = np.float64 if fused else dt
    lo = (wide(start) + wide(step) * i.astype(wide)).astype(dt)
    hi = (wide(end) - wide(step) * (steps - 1 - i).astype(wide)).astype(dt)
    return np.where(i < steps // 2, lo, hi).astype(dt)


def window_grid(size, window, dtype=np.float32):
    """(X, Y) [R] of the window's pixels, row-major within the window: the full grid's values at those pixels"""
    W, H = size
    x0, y0, w, h = (0, 0, W, H) if window is None else window
    if not (0 <= x0 and 0 <= y0 and w >= 1 and h >= 1 and x0 + w <= W and y0 + h <= H):
        raise ValueError(f"window {window} outside the {W} x {H} grid (or empty)")
    xs = linspace(-1.0, 1.0, W, dtype)[x0:x0 + w]
    ys = linspace(1.0, -1.0, H, dtype)[y0:y0 + h]
    return np.tile(xs, h), np.repeat(ys, w)


def jittered_depths(N, ray_start, ray_end, u_jitter, dtype=np.float32):
    """u_jitter [..., N] -> z [..., N] = linspace(start, end, N)[k] + (u - 0.5) * (z_1 - z_0), the linspace fused"""
    dt = np.dtype(dtype).type
    z_lin = linspace(ray_start, ray_end, N, dtype, fused=True)
    step = dt(z_lin[1] - z_lin[0]) if N > 1 else dt(0)
    u = np.asarray(u_jitter).astype(dt)
    return (z_lin + ((u - dt(0.5)) * step).astype(dt)).astype(dt)


def camera_dirs(cam2world, intrinsics, size, window=None, dtype=np.float32):
    """cam2world [B,3,4], intrinsics [B,5] = (kx, ky, cx, cy, zc) -> (origins [B,R,3], dirs [B,R,3], c [B,R,3], n [B,R], X [R], Y [R])"""
    dt = np.dtype(dtype).type
    M = np.asarray(cam2world).astype(dt)
    K = np.asarray(intrinsics).astype(dt)
    X, Y = window_grid(size, window, dtype)
    kx, ky, cx, cy, zc = (K[:, i:i + 1] for i in range(5))               # [B,1]
    with np.errstate(all="ignore"):
        vx = (kx * (X[None] - cx).astype(dt)).astype(dt)                 # [B,R]
        vy = (ky * (Y[None] - cy).astype(dt)).astype(dt)
        vz = np.broadcast_to(zc, vx.shape).astype(dt)
        n = np.sqrt((((vx * vx).astype(dt) + (vy * vy).astype(dt)).astype(dt) + (vz * vz).astype(dt)).astype(dt)).astype(dt)
        c = np.stack([(vx / n).astype(dt), (vy / n).astype(dt), (vz / n).astype(dt)], -1)   # [B,R,3]
        m = lambda j: M[:, None, :, j]                                   # [B,1,3]: column j
        dirs = (((m(0) * c[..., 0:1]).astype(dt) + (m(1) * c[..., 1:2]).astype(dt)).astype(dt) + (m(2) * c[..., 2:3]).astype(dt)).astype(dt)
    origins = np.broadcast_to(M[:, None, :, 3], dirs.shape).copy()
    return origins, dirs, c, n, X, Y


def camera_rays(cam2world, intrinsics, size, window, N, ray_start, ray_end, u_jitter, dtype=np.float32):
    """-> (origins [B,R,3], dirs [B,R,3], z [B,R,N]): fenerf_camera_rays"""
    origins, dirs = camera_dirs(cam2world, intrinsics, size, window, dtype)[:2]
    B, R = dirs.shape[:2]
    z = jittered_depths(N, ray_start, ray_end, np.asarray(u_jitter).reshape(B, R, N), dtype)
    return origins, dirs, z


def reference_intrinsics(fov_degrees, B=1):
    """the reference's camera: (1, 1, 0, 0, -1 / tan(fov / 2)) with zc rounded as its fp32 tensor operation rounds it"""
    zc = (-np.ones(1, dtype=np.float32) / np.float32(np.tan((2 * np.pi * fov_degrees / 360) / 2)))[0]
    return np.tile(np.array([[1, 1, 0, 0, zc]], dtype=np.float32), (B, 1))


def lookat_cam2world(origin, dtype=np.float32):
    """[B,3] camera positions -> [B,3,4]: ray_setup_kernel's look-at basis by its own steps (forward = normalize(normalize(-o)), left =
    normalize(up x f), up' = normalize(f x left), columns (-left, up', -f, o)), each operation rounded in `dtype`"""
    dt = np.dtype(dtype).type
    o = np.asarray(origin).astype(dt)

    def normalize(v):
        n = np.sqrt((((v[:, 0] * v[:, 0]).astype(dt) + (v[:, 1] * v[:, 1]).astype(dt)).astype(dt) + (v[:, 2] * v[:, 2]).astype(dt)).astype(dt))
        return (v / n[:, None]).astype(dt)

    def cross(a, b):
        return np.stack([((a[:, 1] * b[:, 2]).astype(dt) - (a[:, 2] * b[:, 1]).astype(dt)).astype(dt),
                         ((a[:, 2] * b[:, 0]).astype(dt) - (a[:, 0] * b[:, 2]).astype(dt)).astype(dt),
                         ((a[:, 0] * b[:, 1]).astype(dt) - (a[:, 1] * b[:, 0]).astype(dt)).astype(dt)], -1)

    with np.errstate(all="ignore"):
        f = normalize(normalize(-o))
        up = np.zeros_like(f)
        up[:, 1] = 1
        left = normalize(cross(up, f))
        up2 = normalize(cross(f, left))
    return np.stack([-left, up2, -f, o], -1)


def camera_grad_terms(cam2world, intrinsics, size, window, d_origins, d_dirs):
    """The per-ray terms of fenerf_camera_grads in fp64 -> [B, R, 17]: entries 0-11 the terms of d_cam2world (row-major [3][4]), 12-16
    those of d (kx, ky, cx, cy, zc).  d_origins / d_dirs [B,R,3] or None (its terms are zero).  The gradient is the sum over axis 1."""
    f8 = np.float64
    M = np.asarray(cam2world, dtype=f8)
    K = np.asarray(intrinsics, dtype=f8)
    _, _, c, n, X, Y = camera_dirs(M, K, size, window, f8)
    B, R = c.shape[:2]
    t = np.zeros((B, R, 17), dtype=f8)
    if d_origins is not None:
        t[..., [3, 7, 11]] = np.asarray(d_origins, dtype=f8).reshape(B, R, 3)
    if d_dirs is not None:
        dd = np.asarray(d_dirs, dtype=f8).reshape(B, R, 3)
        for i in range(3):
            for j in range(3):
                t[..., 4 * i + j] = dd[..., i] * c[..., j]
        g = np.einsum("bij,bri->brj", M[:, :, :3], dd)
        gv = (g - c * (c * g).sum(-1, keepdims=True)) / n[..., None]
        kx, ky, cx, cy = (K[:, i:i + 1] for i in range(4))
        t[..., 12] = gv[..., 0] * (X[None] - cx)
        t[..., 13] = gv[..., 1] * (Y[None] - cy)
        t[..., 14] = -gv[..., 0] * kx
        t[..., 15] = -gv[..., 1] * ky
        t[..., 16] = gv[..., 2]
    return t
