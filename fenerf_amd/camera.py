"""A free camera for every render entry that takes rays: a camera-to-world matrix and five intrinsics per image, a pixel grid and an
optional window of it.

    cam2world [B,3,4]   columns 0-2: the camera's right, up and backward axes (it looks along -z); column 3: its position
    intrinsics [B,5]    (kx, ky, cx, cy, zc): camera-space direction of pixel (X, Y) in [-1, 1]^2 is normalize(kx (X - cx), ky (Y - cy), zc)

The reference's camera (generators/volumetric_rendering.py: on the unit sphere, looking at the origin, world-up +y, one fov) is
Camera.from_angles(yaw, pitch, fov, size): intrinsics (1, 1, 0, 0, -1 / tan(fov / 2)) and the look-at matrix.

Camera.rays is one HIP launch on a GPU device (fenerf_camera_rays) behind an autograd node whose backward is fenerf_camera_grads:
d_origins, d_dirs -> cam2world.grad, intrinsics.grad.  On the CPU it is the same arithmetic in torch operations."""
import math

import numpy as np
import torch

from . import native
from .generators import volumetric_rendering as VR
from .generators.math_utils_torch import normalize_vecs


def _skew(v):
    """[B,3] -> [B,3,3] cross-product matrices [v]x"""
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    o = torch.zeros_like(x)
    return torch.stack([torch.stack([o, -z, y], -1), torch.stack([z, o, -x], -1), torch.stack([-y, x, o], -1)], -2)


def rotation_exp(rotvec):
    """Rodrigues: [B,3] rotation vectors -> [B,3,3] exp([rotvec]x) = I + A [r]x + B [r]x^2 with A = sin t / t, B = (1 - cos t) / t^2,
    t = |r|.  Below t^2 = 1e-4 the two coefficients are their series in t^2 (three terms: the next one is below 1e-19), so the value and
    the gradient are finite at rotvec = 0, where d R / d r_k = [e_k]x."""
    t2 = (rotvec * rotvec).sum(-1)
    small = t2 < 1e-4
    t2_safe = torch.where(small, torch.ones_like(t2), t2)       # the branch not taken must not put a NaN into the gradient
    t = torch.sqrt(t2_safe)
    a = torch.where(small, 1 - t2 / 6 + t2 * t2 / 120, torch.sin(t) / t)
    b = torch.where(small, 0.5 - t2 / 24 + t2 * t2 / 720, (1 - torch.cos(t)) / t2_safe)
    k = _skew(rotvec)
    eye = torch.eye(3, dtype=rotvec.dtype, device=rotvec.device).expand_as(k)
    return eye + a[:, None, None] * k + b[:, None, None] * (k @ k)


def pixel_grid(size, window, device, dtype=torch.float32):
    """(X, Y) [R] of the window's pixels, row-major: linspace(-1, 1, W)[col], linspace(1, -1, H)[row] with the product rounded on its own,
    as the kernels round it (torch.linspace fuses it)."""
    W, H = size
    x0, y0, w, h = (0, 0, W, H) if window is None else window

    def lin(start, end, steps):
        if steps == 1:
            return torch.full((1,), float(start), dtype=dtype, device=device)
        s, e = torch.tensor(float(start), dtype=dtype, device=device), torch.tensor(float(end), dtype=dtype, device=device)
        step = (e - s) / (steps - 1)
        i = torch.arange(steps, device=device)
        return torch.where(i < steps // 2, s + step * i.to(dtype), e - step * (steps - 1 - i).to(dtype))

    xs, ys = lin(-1, 1, W)[x0:x0 + w], lin(1, -1, H)[y0:y0 + h]
    return xs.repeat(h), ys.repeat_interleave(w)


def rays_torch(cam2world, intrinsics, size, window=None):
    """The torch statement of fenerf_camera_rays' camera part -> (origins [B,R,3], dirs [B,R,3]); differentiable wrt both tensors."""
    X, Y = pixel_grid(size, window, cam2world.device, cam2world.dtype)
    kx, ky, cx, cy, zc = (intrinsics[:, i:i + 1] for i in range(5))
    vx, vy = kx * (X[None] - cx), ky * (Y[None] - cy)
    v = torch.stack([vx, vy, zc.expand_as(vx)], -1)
    c = v / torch.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2]).unsqueeze(-1)
    col = lambda j: cam2world[:, None, :, j]
    dirs = (col(0) * c[..., 0:1] + col(1) * c[..., 1:2]) + col(2) * c[..., 2:3]
    origins = col(3).expand_as(dirs).contiguous()
    return origins, dirs


class CameraRaysFunction(torch.autograd.Function):
    """fenerf_camera_rays -> (origins, dirs, z); backward: fenerf_camera_grads.  The depths carry no graph (the jitter is a draw)."""

    @staticmethod
    def forward(ctx, cam2world, intrinsics, u, size, window, N, ray_start, ray_end):
        origins, dirs, z = native.camera_rays(cam2world, intrinsics, size, window, N, ray_start, ray_end, u)
        ctx.save_for_backward(cam2world, intrinsics)
        ctx.grid = (size, window)
        ctx.mark_non_differentiable(z)
        return origins, dirs, z

    @staticmethod
    def backward(ctx, d_origins, d_dirs, _d_z):
        cam2world, intrinsics = ctx.saved_tensors
        if d_origins is None and d_dirs is None:
            return (None,) * 8
        d_M, d_K = native.camera_grads(cam2world, intrinsics, ctx.grid[0], ctx.grid[1], d_origins, d_dirs)
        return (d_M.reshape(cam2world.shape).to(cam2world.dtype) if ctx.needs_input_grad[0] else None,
                d_K.reshape(intrinsics.shape).to(intrinsics.dtype) if ctx.needs_input_grad[1] else None, None, None, None, None, None, None)


def _angle(v, device):
    return torch.as_tensor(v, dtype=torch.float32).to(device).reshape(-1, 1)


def _z_cam(fov):
    return (-torch.ones(1) / np.tan((2 * math.pi * fov / 360) / 2)).item()      # as the reference's fp32 tensor operation rounds it


class Camera:
    def __init__(self, cam2world, intrinsics, size, window=None):
        W, H = (int(v) for v in size)
        cam2world, intrinsics = torch.as_tensor(cam2world), torch.as_tensor(intrinsics)
        if cam2world.dim() != 3 or tuple(cam2world.shape[1:]) != (3, 4) or tuple(intrinsics.shape) != (cam2world.shape[0], 5):
            raise ValueError(f"Camera: cam2world [B,3,4] and intrinsics [B,5], got {tuple(cam2world.shape)} and {tuple(intrinsics.shape)}")
        if W < 1 or H < 1:
            raise ValueError(f"Camera: size (W, H) = {size}")
        if window is not None:
            x0, y0, w, h = window = tuple(int(v) for v in window)
            if x0 < 0 or y0 < 0 or w < 1 or h < 1 or x0 + w > W or y0 + h > H:
                raise ValueError(f"Camera: the window {window} (x0, y0, w, h) is empty or lies outside the {W} x {H} image")
        self.cam2world, self.intrinsics, self.size, self.window = cam2world, intrinsics, (W, H), window

    # ---- constructors ---------------------------------------------------------------------------------
    @classmethod
    def from_angles(cls, yaw, pitch, fov, size, radius=1.0, roll=0.0, device=None):
        """The reference's camera at (yaw, pitch) = (theta, phi) [B] on the sphere of `radius`, looking at the origin, rolled by `roll`
        radians about its view axis (counter-clockwise as the camera sees it).  At radius = 1, roll = 0: camera_position + the look-at
        rotation, bit for bit.  Angles that require grad stay in the graph."""
        theta, phi = _angle(yaw, device), _angle(pitch, device)
        origin, _, _ = VR.camera_position(theta, phi, radius)
        rot = VR._lookat_rotation(normalize_vecs(-origin))
        if isinstance(roll, torch.Tensor) or roll != 0:
            r = _angle(roll, origin.device).to(origin.dtype)
            right, up = rot[:, :, 0], rot[:, :, 1]
            rot = torch.stack([torch.cos(r) * right + torch.sin(r) * up, torch.cos(r) * up - torch.sin(r) * right, rot[:, :, 2]], -1)
        B = origin.shape[0]
        K = torch.tensor([1, 1, 0, 0, _z_cam(fov)], dtype=torch.float32, device=origin.device).repeat(B, 1)
        return cls(torch.cat([rot, origin.unsqueeze(-1)], -1), K, size)

    @classmethod
    def look_at(cls, eye, target, up, fov, size, device=None):
        """A camera at `eye` [B,3] looking at `target` with `up` roughly upwards (any vector not along the view axis)."""
        vec = lambda v: torch.as_tensor(v, dtype=torch.float32).to(device).reshape(-1, 3)
        eye, target, up = vec(eye), vec(target), vec(up)
        f = normalize_vecs(target - eye)
        right = normalize_vecs(torch.cross(f, up.expand_as(f), dim=-1))
        up2 = torch.cross(right, f, dim=-1)
        B = eye.shape[0]
        K = torch.tensor([1, 1, 0, 0, _z_cam(fov)], dtype=torch.float32, device=eye.device).repeat(B, 1)
        return cls(torch.stack([right, up2, -f, eye.expand_as(f)], -1), K, size)

    # ---- derived cameras ------------------------------------------------------------------------------
    def crop(self, x0, y0, w, h):
        """the same camera restricted to the window [x0, x0 + w) x [y0, y0 + h) of the window it has now (of the image, if none): its
        rays are those rays of the full grid, bit for bit"""
        bx, by = (0, 0) if self.window is None else self.window[:2]
        bw, bh = self.size if self.window is None else self.window[2:]
        if x0 < 0 or y0 < 0 or w < 1 or h < 1 or x0 + w > bw or y0 + h > bh:
            raise ValueError(f"Camera.crop: ({x0}, {y0}, {w}, {h}) is empty or lies outside the {bw} x {bh} window")
        return Camera(self.cam2world, self.intrinsics, self.size, (bx + x0, by + y0, w, h))

    def perturbed(self, rotvec, shift, log_focal=None):
        """R exp([rotvec]x), t + shift, (kx, ky) exp(log_focal): a local SE(3) move (rotvec, shift [B,3]) and a focal change (log_focal
        [B] or None), differentiable in all three; zeros give this camera's values."""
        M = self.cam2world
        rot = M[:, :, :3] @ rotation_exp(rotvec.to(M.dtype))
        pos = M[:, :, 3] + shift.to(M.dtype)
        K = self.intrinsics
        if log_focal is not None:
            s = torch.exp(log_focal.to(K.dtype)).reshape(-1, 1)
            K = torch.cat([K[:, :2] * s, K[:, 2:]], -1)
        return Camera(torch.cat([rot, pos.unsqueeze(-1)], -1), K, self.size, self.window)

    def to(self, device):
        return Camera(self.cam2world.to(device), self.intrinsics.to(device), self.size, self.window)

    def detach(self):
        return Camera(self.cam2world.detach(), self.intrinsics.detach(), self.size, self.window)

    # ---- what a render needs --------------------------------------------------------------------------
    @property
    def batch(self):
        return int(self.cam2world.shape[0])

    @property
    def frame(self):
        """(w, h) of the pixels this camera renders: its window, or the whole image"""
        return self.size if self.window is None else self.window[2:]

    @property
    def requires_grad(self):
        return self.cam2world.requires_grad or self.intrinsics.requires_grad

    def rays(self, N, ray_start, ray_end, draws=VR._DEFAULT_DRAWS):
        """-> (origins [B,R,3], dirs [B,R,3], z [B,R,N]) for the R = w * h pixels of the frame, row-major; one draw: the jitter rand
        [B,R,N,1].  The rays carry the graph to cam2world / intrinsics when those require grad."""
        dev = self.cam2world.device
        w, h = self.frame
        B, R = self.batch, w * h
        u = draws.rand((B, R, N, 1), dev)
        if dev.type == "cuda":
            if torch.is_grad_enabled() and self.requires_grad:
                return CameraRaysFunction.apply(self.cam2world, self.intrinsics, u, self.size, self.window, N, ray_start, ray_end)
            return native.camera_rays(self.cam2world, self.intrinsics, self.size, self.window, N, ray_start, ray_end, u)
        z_lin = torch.linspace(ray_start, ray_end, N, device=dev)
        step = (z_lin[1] - z_lin[0]) if N > 1 else torch.zeros((), device=dev)
        z = z_lin.reshape(1, 1, N) + (u.squeeze(-1) - 0.5) * step
        origins, dirs = rays_torch(self.cam2world, self.intrinsics, self.size, self.window)
        return origins, dirs.contiguous(), z.contiguous()
