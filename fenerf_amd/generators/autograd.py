"""Differentiable final compositing: torch.autograd.Function wrappers whose forward AND backward are the
HIP kernels behind fenerf_composite / fenerf_merge_composite / fenerf_composite_backward (include/fenerf.h) -- what
torch autograd derives for fancy_integration (volumetric_rendering.py:23-50) after the cat / sort / gather of
generators.py:508-519.  Depth is returned detached (the reference's losses never read it) unless the caller asks for a differentiable
depth: the *DepthFunction variants of the nodes below (`depth_grad = True` on the node class), whose backward is
fenerf_composite_backward_outputs / fenerf_render_backward_outputs; z values and noise are constants of the graph, exactly as in the
reference where they are produced under torch.no_grad()."""
import torch

from .. import _lib, native
from ..siren import autograd as _siren_autograd


class ImageLayoutFunction(torch.autograd.Function):
    """pixels [B, S*S, C] in [0, 1] -> the image the generators return, [B, C, S, S] * 2 - 1 (generators.py:519-521: reshape,
    permute(0, 3, 1, 2).contiguous(), * 2 - 1), as ONE launch forward and one backward instead of three and three (2 x exact in fp32, so
    the fused a + 2 b rounds once like the reference's (2 b) - 1: bit-identical).  Values only; not twice differentiable."""

    @staticmethod
    def forward(ctx, pixels, B, S):
        v = pixels.reshape(B, S, S, -1).permute(0, 3, 1, 2)
        out = torch.empty(v.shape, dtype=pixels.dtype, device=pixels.device)
        torch.add(torch.tensor(-1.0, dtype=pixels.dtype), v, alpha=2.0, out=out)       # a 0-dim CPU tensor is a scalar operand
        ctx.shape = pixels.shape
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        d = torch.empty((g.shape[0], g.shape[2], g.shape[3], g.shape[1]), dtype=g.dtype, device=g.device)
        torch.mul(g.permute(0, 2, 3, 1), 2.0, out=d)
        return d.reshape(ctx.shape), None, None


def _depth_output(ctx, depth):
    """A node's depth output: non-differentiable, as ever, unless the node class says `depth_grad = True` -- then an unused output's
    gradient (depth's or rgb's) arrives as None, costs nothing, and reaches the library as a NULL pointer"""
    ctx.depth_grad = bool(ctx._forward_cls.depth_grad)
    if ctx.depth_grad:
        ctx.set_materialize_grads(False)
    else:
        ctx.mark_non_differentiable(depth)


def _upstream(ctx, g_rgb, g_depth, rgb_shape):
    """-> (g_rgb, g_depth) as the composite backward takes them: contiguous fp32 or None; without depth_grad exactly what the node passed before"""
    if not ctx.depth_grad:
        return g_rgb, None
    return (g_rgb.contiguous().float().reshape(rgb_shape) if g_rgb is not None else None,
            g_depth.contiguous().float().reshape(-1) if g_depth is not None else None)


class CompositeFunction(torch.autograd.Function):
    depth_grad = False      # CompositeDepthFunction: depth is a differentiable output too

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)   # under autocast (the reference's training loop) inputs arrive as fp16
    def forward(ctx, rows, z, noise, opts):
        rgb, depth, _, _ = native.composite(rows, z, noise, opts, want_weights=False, want_wsum=False)
        ctx.opts = opts
        ctx.save_for_backward(rows, z, noise if noise is not None else rows.new_empty(0))
        _depth_output(ctx, depth)
        return rgb, depth

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g_rgb, g_depth):
        rows, z, noise = ctx.saved_tensors
        lead, M, C = rows.shape[:-2], rows.shape[-2], rows.shape[-1]
        g_rgb, g_depth = _upstream(ctx, g_rgb, g_depth, (-1, C - 1))
        if g_rgb is None and g_depth is None:
            return None, None, None, None
        d = native.composite_backward(g_rgb.reshape(-1, C - 1) if g_rgb is not None else None, rows.reshape(-1, M, C), z.reshape(-1, M), ctx.opts,
                                      noise=noise.reshape(-1, M) if noise.numel() else None, g_depth=g_depth)
        return d.reshape(*lead, M, C), None, None, None


class CompositeDepthFunction(CompositeFunction):
    """CompositeFunction whose depth output carries the graph too (backward: fenerf_composite_backward_outputs)."""
    depth_grad = True


class CompositeOutputsFunction(torch.autograd.Function):
    """rows [..., M, C], z [..., M], noise or None -> (rgb [..., C-1], depth [...], weights [..., M] in sorted order, wsum [...]): every
    output of fancy_integration (volumetric_rendering.py:23-50; wsum = sum of the weights before the last_back adjustment, :40)
    differentiable wrt the rows -- the node behind the drop-in volumetric_rendering.fancy_integration under grad.  Values are
    native.composite's; backward is fenerf_composite_backward_outputs with NULL for every output the loss does not read."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, rows, z, noise, opts):
        rgb, depth, weights, wsum = native.composite(rows, z, noise, opts)
        ctx.opts = opts
        ctx.save_for_backward(rows, z, noise if noise is not None else rows.new_empty(0))
        ctx.set_materialize_grads(False)
        return rgb, depth, weights, wsum

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g_rgb, g_depth, g_weights, g_wsum):
        if g_rgb is None and g_depth is None and g_weights is None and g_wsum is None:
            return None, None, None, None
        rows, z, noise = ctx.saved_tensors
        lead, M, C = rows.shape[:-2], rows.shape[-2], rows.shape[-1]
        f = lambda g, *shape: g.contiguous().float().reshape(*shape) if g is not None else None
        d = native.composite_backward(f(g_rgb, -1, C - 1), rows.reshape(-1, M, C), z.reshape(-1, M), ctx.opts,
                                      noise=noise.reshape(-1, M) if noise.numel() else None, g_depth=f(g_depth, -1), g_weights=f(g_weights, -1, M),
                                      g_wsum=f(g_wsum, -1))
        return d.reshape(*lead, M, C), None, None, None


class MergeCompositeFunction(torch.autograd.Function):
    """fine / coarse [BR,N,C] with their own depths [BR,N] -> (rgb [BR,C-1], depth [BR])."""
    depth_grad = False      # MergeCompositeDepthFunction: depth is a differentiable output too

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)   # under autocast (the reference's training loop) inputs arrive as fp16
    def forward(ctx, fine, coarse, z_fine, z_coarse, noise, opts):
        rgb, depth, _, _, _ = native.merge_composite(fine, coarse, z_fine, z_coarse, noise, opts, want_weights=False,
                                                     want_wsum=False, want_z=False)
        ctx.opts = opts
        ctx.save_for_backward(fine, coarse, z_fine, z_coarse, noise if noise is not None else fine.new_empty(0))
        _depth_output(ctx, depth)
        return rgb, depth

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g_rgb, g_depth):
        fine, coarse, z_fine, z_coarse, noise = ctx.saved_tensors
        g_rgb, g_depth = _upstream(ctx, g_rgb, g_depth, (fine.shape[0], fine.shape[-1] - 1))
        if g_rgb is None and g_depth is None:
            return (None,) * 6
        d_f, d_c = native.composite_backward(g_rgb, fine, z_fine, ctx.opts, rows_b=coarse, z_b=z_coarse,
                                             noise=noise if noise.numel() else None, g_depth=g_depth)
        return d_f, d_c, None, None, None, None


class MergeCompositeDepthFunction(MergeCompositeFunction):
    """MergeCompositeFunction whose depth output carries the graph too (backward: fenerf_composite_backward_outputs)."""
    depth_grad = True


def _hierarchical_forward(ctx, module, opts, copts, lock_view, origins, dirs, z_c, u, noise_c, noise_f, fg, pg, fa, pa, params, film_only):
    """Forward of the hierarchical render node (both variants below): coarse forward-save -> (no-grad) coarse weights -> resampled depths
    -> fine forward-save -> merged composite; saves what the backward needs on ctx."""
    dev = origins.device
    nat = module.native_differentiable(dev)
    B, R, N = z_c.shape
    C, H = nat.C, nat.spec["hidden_dim"]
    L = nat.spec["n_geo"] + nat.spec["n_color"]
    P = R * N
    Pp = (P + 31) // 32 * 32                      # whole 32-point tiles per image; pad rows get no gradient
    G = nat.spec["grid_ch"]

    def samples(z):                               # [B,R,N] depths -> padded [B,Pp,3] points
        pts = (origins.unsqueeze(2) + dirs.unsqueeze(2) * z.unsqueeze(-1)).reshape(B, P, 3)   # generators.py:504
        return torch.cat([pts, pts[:, -1:].expand(-1, Pp - P, -1)], 1) if Pp != P else pts

    rd = None
    if not lock_view:
        rd = dirs.unsqueeze(2).expand(-1, -1, N, -1).reshape(B, P, 3)
        rd = (torch.cat([rd, rd[:, -1:].expand(-1, Pp - P, -1)], 1) if Pp != P else rd).contiguous()
    pts2 = torch.empty((2 * B, Pp, 3), dtype=torch.float32, device=dev)
    out2 = torch.empty((2 * B, Pp, C), dtype=torch.float32, device=dev)
    # the tape's format is fixed here: the 16-bit tape (siren.grad_precision = "tape16") for backward passes that take weight gradients,
    # the fp32 tape for FiLM-only ones (inversion); `film_only` as the backward will compute it
    fmt = ctx.tape_format = module.tape_format(nat, film_only=film_only)
    half = nat.tape_words_per_point(fmt) * B * Pp
    tape2 = torch.empty(half + nat.tape_floats(B * Pp, fmt), dtype=torch.float32, device=dev)   # pass 1 | pass 2 + slack
    tape_e2 = torch.empty((2 * B * Pp, 32), dtype=torch.float32, device=dev) if G else None
    pts2[:B] = samples(z_c)
    nat.siren_forward_save(pts2[:B], rd, fg, pg, fa, pa, out=out2[:B], tape=tape2[:half], tape_e=tape_e2[:B * Pp] if G else None, tape_format=fmt)
    coarse = out2[:B, :P].reshape(B * R, N, C)
    zc = z_c.reshape(B * R, N)
    _, _, w_c, _ = native.composite(coarse, zc, noise_c, copts, want_wsum=False)
    z_f = native.resample(zc, w_c, u)
    pts2[B:] = samples(z_f.reshape(B, R, N))
    nat.siren_forward_save(pts2[B:], rd, fg, pg, fa, pa, out=out2[B:], tape=tape2[half:], tape_e=tape_e2[B * Pp:] if G else None, tape_format=fmt)
    fine = out2[B:, :P].reshape(B * R, N, C)
    rgb, depth, _, _, _ = native.merge_composite(fine, coarse, z_f, zc, noise_f, opts, want_weights=False, want_wsum=False, want_z=False)
    ctx.module, ctx.nat, ctx.opts, ctx.dims = module, nat, opts, (B, R, N, P, Pp)
    ctx.pack_generation = nat.pack_generation
    empty = origins.new_empty(0)
    ctx.save_for_backward(pts2, rd if rd is not None else empty, fg, pg, fa, pa, out2, tape2, tape_e2 if G else empty, z_f, zc,
                          noise_f if noise_f is not None else empty, *params)
    depth = depth.reshape(B, R)
    _depth_output(ctx, depth)
    return rgb.reshape(B, R, C - 1), depth


# The render runs through fenerf_render_forward_save / fenerf_render_backward (round 5: chunk planning, workspaces, launch order and gradient
# sums live behind the C-ABI; include/fenerf.h) -- and, in its two-node (DistributedDataParallel) form, fenerf_render_backward_stage 1 / 2.  The
# Python below it is the round-4 orchestration of the same kernels, kept for the two-stream experiment (siren/autograd.py OVERLAP_WGRAD) and
# as the reference the tests compare the library's paths with bit for bit.
USE_RENDER_ABI = True


def _abi_forward(ctx, module, opts, lock_view, origins, dirs, z_c, u, noise_c, noise_f, fg, pg, fa, pa, params, film_only):
    """Forward of the render node (one-node form and render stage of the two-node form) through fenerf_render_forward_save; saves what
    fenerf_render_backward / fenerf_render_backward_stage need on ctx.  `film_only` as the backward will compute it (the tape's format)."""
    nat = module.native_differentiable(origins.device)
    B, R, N = z_c.shape
    ctx.tape_format = module.tape_format(nat, film_only=film_only)
    rgb, depth, save = nat.render_forward_save(origins, dirs, z_c, u, noise_c, noise_f, fg, pg, fa, pa, opts, lock_view=lock_view,
                                               tape_format=ctx.tape_format)
    ctx.module, ctx.nat, ctx.opts, ctx.dims, ctx.lock_view = module, nat, opts, (B, R, N), lock_view
    ctx.pack_generation = nat.pack_generation
    ctx.save_for_backward(save, z_c, noise_f if noise_f is not None else origins.new_empty(0), *params)
    _depth_output(ctx, depth)
    return rgb, depth


def _python_composite_backward(nat, opts, dims, g_rgb, rd, film, out2, z_f, zc, noise_f, g_depth=None):
    """Start of the backward of the Python orchestration, over what _hierarchical_forward saved: the composite backward of both passes
    -> (d_out2 [2B,Pp,C], film2, rd2): the chain's upstream gradient, FiLM parameters and view directions over 2B pass-major "images"
    (image b' = pass * B + b: coarse | fine)."""
    B, R, N, P, Pp = dims
    C = nat.C
    fine, coarse = out2[B:, :P].reshape(B * R, N, C), out2[:B, :P].reshape(B * R, N, C)
    noise = noise_f if noise_f.numel() else None
    g_rgb = g_rgb.reshape(B * R, C - 1) if g_rgb is not None else None         # None: a loss that reads the depth only (g_depth given)
    if Pp == P:     # whole tiles per image: the composite backward writes the chain's input directly
        d_out2 = torch.empty_like(out2)
        native.composite_backward(g_rgb, fine, z_f, opts, rows_b=coarse, z_b=zc, noise=noise,
                                  out_a=d_out2[B:].view(B * R, N, C), out_b=d_out2[:B].view(B * R, N, C), g_depth=g_depth)
    else:
        d_f, d_c = native.composite_backward(g_rgb, fine, z_f, opts, rows_b=coarse, z_b=zc, noise=noise, g_depth=g_depth)
        d_out2 = torch.zeros((2 * B, Pp, C), dtype=torch.float32, device=out2.device)
        d_out2[:B, :P] = d_c.reshape(B, P, C)
        d_out2[B:, :P] = d_f.reshape(B, P, C)
    return d_out2, [torch.cat([t, t]) for t in film], torch.cat([rd, rd]) if rd.numel() else None


def check_ray_grads_supported(module):
    """Rays that require grad: refuse the gradient tiers whose backward chunks write the bf16 d(theta) dump (nothing for the input-gradient
    pass to read) -- up front, in the forward."""
    if getattr(module, "grad_precision", "f32") in ("amp", "amp16"):
        raise NotImplementedError(f"fenerf_amd: gradients wrt the rays (camera pose) are not available with siren.grad_precision = "
                                  f"{module.grad_precision!r}; use grad_precision 'f32' or 'tape16'")


def rays_require_grad(origins, dirs):
    return torch.is_grad_enabled() and (origins.requires_grad or dirs.requires_grad)


class HierarchicalRenderFunction(torch.autograd.Function):
    """The whole differentiable hierarchical render of generators.py:479-519 as ONE autograd node: coarse SIREN pass ->
    (no-grad) coarse weights -> resampled depths -> fine SIREN pass -> merged composite.  Both passes write their tapes into
    the two halves of one buffer, so the backward is one composite-backward, ONE chain launch and ONE set of weight-gradient
    launches over 2B "images" (pass-major) -- instead of two of each plus 34 tensor additions when the passes are separate
    SirenFunction nodes.  Inputs: rays (origins / dirs [B,R,3], coarse depths z_c [B,R,N]), the caller's draws (u [B*R,N],
    noise_c / noise_f or None), composite options, raw FiLM parameters, then module._render_params().
    -> (rgb [B,R,C-1], depth [B,R])."""
    depth_grad = False      # HierarchicalRenderDepthFunction: depth is a differentiable output too

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, module, opts, copts, lock_view, origins, dirs, z_c, u, noise_c, noise_f, fg, pg, fa, pa, *params):
        film_only = not any(ctx.needs_input_grad[14:])
        if ctx.needs_input_grad[4] or ctx.needs_input_grad[5]:
            # Rays that require grad (a camera pose under optimisation).  The backward reads the chunks' fp32 d(theta) dumps once more
            # (fenerf_siren_input_grads); every tape format tape_format() picks below leaves one -- a FiLM-only step simply takes the
            # dumping chain -- except the bf16 dumps of the AMP tiers.
            check_ray_grads_supported(module)
        ctx.abi = USE_RENDER_ABI and not (_siren_autograd.OVERLAP_WGRAD)
        if not ctx.abi:
            return _hierarchical_forward(ctx, module, opts, copts, lock_view, origins, dirs, z_c, u, noise_c, noise_f, fg, pg, fa, pa, params, film_only=film_only)
        return _abi_forward(ctx, module, opts, lock_view, origins, dirs, z_c, u, noise_c, noise_f, fg, pg, fa, pa, params, film_only)

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g_rgb, g_depth):
        module, nat, opts = ctx.module, ctx.nat, ctx.opts
        _siren_autograd.check_same_weights(ctx, nat)
        need = ctx.needs_input_grad
        film_only = not any(need[14:])
        if ctx.depth_grad:
            g_rgb, g_depth = _upstream(ctx, g_rgb, g_depth, (ctx.dims[0], ctx.dims[1], nat.C - 1))
            if g_rgb is None and g_depth is None:
                return (None,) * len(need)
        else:
            g_depth = None
        if ctx.abi:
            B, R, N = ctx.dims
            save, z_c, noise_f, *params = ctx.saved_tensors
            nat.set_grid_grad_mode(_siren_autograd.deterministic_grid(module))
            ray_grads = None
            if need[4] or need[5]:
                w_geo, w_col = _siren_autograd.film_layer_weights(module, params)
                ray_grads = (w_geo[0], w_col[0], need[4], need[5])
            r, g_grid = nat.render_backward(B, R, N, save, z_c, noise_f if noise_f.numel() else None, opts,
                                            g_rgb.contiguous().float() if g_rgb is not None else None, film_only,
                                            lock_view=ctx.lock_view, tape_format=ctx.tape_format,
                                            weights=_siren_autograd.film_layer_weights(module, params) if ctx.tape_format else None,
                                            chunk_points=_siren_autograd.BACKWARD_CHUNK_POINTS, film_sums_budget_bytes=_siren_autograd.FILM_SUMS_BUDGET_BYTES,
                                            ray_grads=ray_grads, g_depth=g_depth)
            return (None,) * 4 + (r.get("d_origins"), r.get("d_dirs")) + (None,) * 4 \
                + _siren_autograd.grads_tail(module, nat, params, r, need, 10, film_only, d_grid_ncdhw=g_grid)
        B, R, N, P, Pp = ctx.dims
        pts2, rd, fg, pg, fa, pa, out2, tape2, tape_e2, z_f, zc, noise_f, *params = ctx.saved_tensors
        d_out2, film2, rd2 = _python_composite_backward(nat, opts, ctx.dims, g_rgb, rd, (fg, pg, fa, pa), out2, z_f, zc, noise_f, g_depth)
        rows = _siren_autograd.begin_grid_gradient(module, nat, 2 * B * Pp, film_only)
        input_grads = None
        if need[4] or need[5]:      # per-sample d points / d view directions of both passes, chunk by chunk, then one reduction per ray
            w_geo, w_col = _siren_autograd.film_layer_weights(module, params)
            new = lambda: torch.empty((2 * B, Pp, 3), dtype=torch.float32, device=pts2.device)
            input_grads = _siren_autograd.InputGrads(w_geo[0], w_col[0], new(), new() if (need[5] and rd2 is not None) else None)
        r, d_grid = _siren_autograd.chunked_backward(nat, 2 * B, Pp, film2, pts2, rd2, out2, d_out2, tape2,
                                                  tape_e2 if tape_e2.numel() else None, film_only, tape_format=ctx.tape_format,
                                                  weights=_siren_autograd.film_layer_weights(module, params) if ctx.tape_format else None,
                                                  input_grads=input_grads, grid_rows=rows)
        if rows is not None:
            d_grid = rows.reduce(nat)
        d_o = d_d = None
        if input_grads is not None:
            d_o, d_d = native.ray_grads(input_grads.d_points, input_grads.d_dirs, zc.reshape(B, R, N), z_f, want_origins=need[4], want_dirs=need[5])
        return (None,) * 4 + (d_o, d_d) + (None,) * 4 + _siren_autograd.grads_tail(module, nat, params, r, need, 10, film_only, B=B, d_grid_cl=d_grid)


class HierarchicalRenderDepthFunction(HierarchicalRenderFunction):
    """HierarchicalRenderFunction whose depth output carries the graph too: a loss may read the depth map (a depth target, a second view's
    geometry) beside or instead of the pixels.  backward: fenerf_render_backward_outputs (C-ABI route) / the composite backward's
    depth term (Python orchestration); everything behind the composite backward is the same."""
    depth_grad = True


# ----------------------------------------------------------------------------------------------------------------------------------
# Exact sparsity of the backward pass (round 6; opt-in per module, `siren.sparse_backward = True`).  A sample whose row of upstream
# gradients is ALL ZERO contributes exact zeros to every gradient of the step -- and under the reference's relu clamp that is every
# sample with sigma + noise <= 0: its compositing weight alpha T is 0, so the colour / label channels take 0 * g, and relu' = 0 stops
# the density gradient (volumetric_rendering.py:36-47; torch autograd multiplies the same zeros through the whole SIREN).  In a density
# field that is mostly empty space that is most samples: 89 % of the coarse samples of the bench model (tools/exp/empty_fraction.py).
# So the forward here is the NO-GRAD render kept stage by stage (its 22 outputs per sample are all it saves: 69 MB instead of a 9-GB
# tape), and the backward runs composite-backward over all samples, keeps the samples with a non-zero gradient row (per image, padded
# to whole 32-point tiles with samples whose rows are zero anyway), and only THOSE go through forward-save, the chain and the
# weight-gradient kernels.  Same gradients as the dense node up to the order of the sums; nothing is approximated, nothing is skipped
# that the reference's arithmetic would not multiply by zero.  With another clamp mode (softplus) every row is non-zero and this is
# the dense backward plus a re-evaluation (`siren.sparse_backward = "auto"` then falls back to the dense node, below).  The backward does not wait for the device: the length of its buffers is a bound the FORWARD
# computes (samples with sigma + max|noise| std > 0, + one per ray with last_back: a row is non-zero only if alpha > 0), fetched
# asynchronously; which samples are kept is decided on the device from the rows themselves.
# A differentiable depth (the Sparse*DepthFunction variants) leaves that bound as it is: gradients of depth / weights / wsum reach a
# row's density only through act'(sigma + noise) (`dact` in composite_backward_kernel), which is 0 -- a selected zero -- at a clamped
# sample, and they never reach its colour channels (those are w'_k g_rgb_c whatever else the loss reads).  So the rows that can be
# non-zero are the same rows.
# ----------------------------------------------------------------------------------------------------------------------------------
class SparseHierarchicalRenderFunction(torch.autograd.Function):
    """HierarchicalRenderFunction's signature and results; see the block comment above."""
    depth_grad = False      # SparseHierarchicalRenderDepthFunction: depth is a differentiable output too

    # report and check state of the LAST sparse backward of the process (either sparse node)
    last_kept = None            # (kept samples: a device scalar -- read it after the step, all samples)
    last_groups = None          # [(images, slots per image)] of its launch groups
    _pending = None             # (pinned overflow flag, event of its copy) not yet read

    @staticmethod
    def _check_overflow(overflowed):
        """Deferred assertion of the sparse backward's buffer bound: the flag of THIS call is copied to the host without waiting and read by the
        next call (or by SparseHierarchicalRenderFunction.verify()); a set flag means samples were dropped -- an error, never a silent result."""
        SparseHierarchicalRenderFunction.verify(wait=False)
        flag = torch.empty((), dtype=torch.bool, pin_memory=True)
        flag.copy_(overflowed != 0, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        SparseHierarchicalRenderFunction._pending = (flag, ev)

    @staticmethod
    def verify(wait=True):
        if SparseHierarchicalRenderFunction._pending is None:
            return
        flag, ev = SparseHierarchicalRenderFunction._pending
        if not wait and not ev.query():
            return
        ev.synchronize()
        SparseHierarchicalRenderFunction._pending = None
        if bool(flag):
            raise RuntimeError("fenerf_amd: sparse backward: more samples carried a non-zero gradient row than the forward's bound allowed for; "
                               "the gradients of that backward pass are incomplete (please report; siren.sparse_backward = False avoids it)")

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, module, opts, copts, lock_view, origins, dirs, z_c, u, noise_c, noise_f, fg, pg, fa, pa, *params):
        nat = module.native_differentiable(origins.device)
        B, R, N = z_c.shape
        C = nat.C
        coarse = nat.siren_forward_rays(origins, dirs, z_c, fg, pg, fa, pa, lock_view=lock_view).reshape(B * R, N, C)
        zc = z_c.reshape(B * R, N)
        _, _, w_c, _ = native.composite(coarse, zc, noise_c, copts, want_wsum=False)
        z_f = native.resample(zc, w_c, u)
        fine = nat.siren_forward_rays(origins, dirs, z_f.reshape(B, R, N), fg, pg, fa, pa, lock_view=lock_view).reshape(B * R, N, C)
        rgb, depth, _, _, _ = native.merge_composite(fine, coarse, z_f, zc, noise_f, opts, want_weights=False, want_wsum=False, want_z=False)
        P = R * N
        _record_bound(ctx, opts, torch.cat([coarse[..., -1].reshape(B, P), fine[..., -1].reshape(B, P)], 1), noise_f, B, R)
        ctx.module, ctx.nat, ctx.opts, ctx.dims, ctx.lock_view = module, nat, opts, (B, R, N), lock_view
        ctx.pack_generation = nat.pack_generation
        ctx.save_for_backward(origins, dirs, zc, z_f, coarse, fine, noise_f if noise_f is not None else origins.new_empty(0), fg, pg, fa, pa, *params)
        depth = depth.reshape(B, R)
        _depth_output(ctx, depth)
        return rgb.reshape(B, R, C - 1), depth

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g_rgb, g_depth):
        module, nat, opts = ctx.module, ctx.nat, ctx.opts
        _siren_autograd.check_same_weights(ctx, nat)
        need = ctx.needs_input_grad
        B, R, N = ctx.dims
        origins, dirs, zc, z_f, coarse, fine, noise_f, fg, pg, fa, pa, *params = ctx.saved_tensors
        if ctx.depth_grad:
            g_rgb, g_depth = _upstream(ctx, g_rgb, g_depth, (B * R, nat.C - 1))
            if g_rgb is None and g_depth is None:
                return (None,) * len(need)
        else:
            g_rgb, g_depth = g_rgb.contiguous().float().reshape(B * R, nat.C - 1), None
        d_f, d_c = native.composite_backward(g_rgb, fine, z_f, opts, rows_b=coarse, z_b=zc, noise=noise_f if noise_f.numel() else None,
                                             g_depth=g_depth)
        return _sparse_siren_backward(ctx, module, nat, need, B, R, N, 2, d_c, d_f, zc, z_f, origins, dirs, (fg, pg, fa, pa), params,
                                      [g for g in (g_rgb, g_depth) if g is not None])


class SparseHierarchicalRenderDepthFunction(SparseHierarchicalRenderFunction):
    """SparseHierarchicalRenderFunction whose depth output carries the graph too (g_depth goes to the composite backward it already calls)."""
    depth_grad = True


def _record_bound(ctx, opts, sig, noise, B, R):
    """How many samples of an image CAN carry a non-zero gradient row -- computed in the forward so that the backward never waits for the
    device: a row is non-zero only if alpha > 0, i.e. (relu clamp) sigma + noise * std > 0; the noise of a sample is the draw of its SORTED
    position, so the bound takes the largest |draw| of the render; `last_back` adds the ray's last sample (its colour row takes the residual
    weight whatever its density).  NaN densities count.  The softplus clamp keeps every sample.  sig [B, samples of the image]."""
    if opts.clamp_mode == _lib.CLAMP["relu"]:
        if noise is not None and opts.noise_std != 0:
            sig = sig + noise.abs().max() * opts.noise_std
        cap = (~(sig <= 0)).sum(1) + (R if opts.last_back else 0)                          # per image
        ctx.cap_host = torch.empty((B,), dtype=torch.long, pin_memory=True)
        ctx.cap_host.copy_(cap, non_blocking=True)
        ctx.cap_ready = torch.cuda.Event()
        ctx.cap_ready.record()
    else:
        ctx.cap_host, ctx.cap_ready = None, None


def _sparse_siren_backward(ctx, module, nat, need, B, R, N, passes, d_c, d_f, zc, z_f, origins, dirs, film, params, upstream):
    """The SIREN part of a sparse backward: d_c (/ d_f) [B*R, N, C] = gradients wrt the outputs of the pass(es) -> the autograd node's
    return tuple (10 Nones, four FiLM gradients, parameter gradients).  passes = 2: coarse | fine; 1: d_f = z_f = None.  upstream: the
    node's upstream gradients (g_rgb, and g_depth of a differentiable depth) -- only asked whether they are finite."""
    fg, pg, fa, pa = film
    S = passes * R * N                                                          # samples per image
    dev = origins.device
    # the buffer lengths come from the forward's per-image bounds (that copy finished long ago), so nothing here waits for the device
    if ctx.cap_ready is not None:
        ctx.cap_ready.synchronize()
        caps = [min(S, int(c)) for c in ctx.cap_host.tolist()]
    else:
        caps = [S] * B
    # whole 32-point tiles; beyond 64 Ki samples whole blocks of 2,048 (<= 3 % more zero rows): the buffer lengths of consecutive steps then
    # repeat, and the caching allocator serves them from the blocks it has instead of growing by a new size every step (400 steps with 397
    # different lengths: 34 GB reserved for 0.6 GB allocated, tools/exp/sparse_soak.py)
    caps = [min(-(-S // 32) * 32, -(-c // 2048) * 2048) if c > 65536 else max(32, (c + 31) // 32 * 32) for c in caps]
    # images that keep similar numbers of samples share a launch group (padded to the group's fullest image); a batch of one dense and
    # five nearly empty images is not padded to six dense ones
    groups = plan_sparse_groups(caps, torch.cuda.get_device_properties(dev).multi_processor_count)
    sparse_auto_observe(module, sum(len(g) * c for g, c in groups) / (S * B))
    whole = len(groups) == 1
    perm = None if whole else torch.tensor([b for g, _ in groups for b in g], dtype=torch.long).pin_memory().to(dev, non_blocking=True)
    film_only = not any(need[14:])
    fmt = module.tape_format(nat, film_only=film_only)
    weights = _siren_autograd.film_layer_weights(module, params) if fmt else None
    total, d_grid, film_rows, kept, flags, first = None, None, [], [], [], 0
    # deterministic grid gradient: the kept rows of every group, reduced once at the scale of the DENSE backward's row count (its padded
    # points per image per pass) -- the zero rows the dense backward has beside them add nothing, so dense and sparse get the same bits
    rows = _siren_autograd.begin_grid_gradient(module, nat, passes * B * (-(-(R * N) // 32) * 32), film_only)
    for g, cap in groups:
        ids = None if whole else perm[first:first + len(g)]
        first += len(g)
        # kept samples (a row with a non-zero -- NaN != 0: a broken row is kept, not hidden) first, in sample order, coarse pass first; the
        # slots beyond an image's count repeat its first sample with a zero row (native.sparse_select: three launches)
        pts, rd, d_sel, counts = native.sparse_select(d_c, d_f, zc, z_f, origins, dirs, cap, want_dirs=not ctx.lock_view, images=ids)
        film_g = (fg, pg, fa, pa) if whole else tuple(t.index_select(0, ids) for t in (fg, pg, fa, pa))
        out, tape, tape_e = nat.siren_forward_save(pts, rd, *film_g, tape_format=fmt)
        r, d_grid = _siren_autograd.chunked_backward(nat, len(g), cap, film_g, pts, rd, out, d_sel, tape, tape_e, film_only, tape_format=fmt,
                                                  weights=weights, d_grid=d_grid, grid_rows=rows)
        del out, tape, tape_e, d_sel
        film_rows.append([r[k] for k in _siren_autograd.FILM_KEYS])
        if not film_only:
            if total is None:
                total = r
            else:
                _siren_autograd._add_all(_siren_autograd._flat(total, _siren_autograd.FILM_KEYS), _siren_autograd._flat(r, _siren_autograd.FILM_KEYS))
        kept.append(counts[:len(g)].sum())
        flags.append(counts[len(g)])
    # (a count above its bound would mean the bound's argument is wrong: checked without waiting, reported by the next backward)
    if rows is not None:
        d_grid = rows.reduce(nat)
    # A non-finite UPSTREAM gradient makes every row of its ray non-zero (0 * NaN), clamped samples included -- more rows than the
    # forward's bound, which knows the densities only.  That is no error of the bound: the reference's gradients of such a step are
    # non-finite too (a GradScaler skips it).  So the flag is raised only while the upstream gradient is finite; otherwise the rows that
    # were dropped are made up for by a NaN added to every gradient this node returns (all on the device, nothing waits).
    overflowed = (flags[0] if whole else torch.stack(flags).max()) != 0
    g_ok = torch.isfinite(upstream[0]).all()
    for g in upstream[1:]:
        g_ok = g_ok & torch.isfinite(g).all()
    SparseHierarchicalRenderFunction._check_overflow(overflowed & g_ok)
    poison = torch.where(overflowed & ~g_ok, float("nan"), 0.0)
    SparseHierarchicalRenderFunction.last_kept = (kept[0] if whole else torch.stack(kept).sum(), S * B)            # for reports (a device scalar: read it after the step)
    SparseHierarchicalRenderFunction.last_groups = [(list(g), c) for g, c in groups]
    if whole:
        film_g = film_rows[0]
    else:       # rows back into image order
        film_g = [torch.cat([rows[i] for rows in film_rows], 0).index_select(0, torch.argsort(perm)) for i in range(len(_siren_autograd.FILM_KEYS))]
    r = {**(total or {}), **dict(zip(_siren_autograd.FILM_KEYS, film_g))}         # the groups' summed weight gradients, every image's FiLM rows
    grads = _siren_autograd.grads_tail(module, nat, params, r, need, 10, film_only, d_grid_cl=d_grid)
    torch._foreach_add_([t for t in grads if t is not None], poison)
    return (None,) * 10 + grads


class SparseSinglePassRenderFunction(torch.autograd.Function):
    """The render WITHOUT importance resampling (hierarchical_sample False: generators.py:479-483 + :519 on the coarse samples -- the
    reference's inversion renders, inverse_render_double_semantic.py:225-247) as one node with the exact-sparsity backward of the block
    comment above: SparseHierarchicalRenderFunction's signature (u and noise_c unused) and results."""
    depth_grad = False      # SparseSinglePassRenderDepthFunction: depth is a differentiable output too

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, module, opts, copts, lock_view, origins, dirs, z_c, u, noise_c, noise_f, fg, pg, fa, pa, *params):
        nat = module.native_differentiable(origins.device)
        B, R, N = z_c.shape
        C = nat.C
        rows = nat.siren_forward_rays(origins, dirs, z_c, fg, pg, fa, pa, lock_view=lock_view).reshape(B * R, N, C)
        zc = z_c.reshape(B * R, N)
        rgb, depth, _, _ = native.composite(rows, zc, noise_f, opts, want_weights=False, want_wsum=False)
        _record_bound(ctx, opts, rows[..., -1].reshape(B, R * N), noise_f, B, R)
        ctx.module, ctx.nat, ctx.opts, ctx.dims, ctx.lock_view = module, nat, opts, (B, R, N), lock_view
        ctx.pack_generation = nat.pack_generation
        ctx.save_for_backward(origins, dirs, zc, rows, noise_f if noise_f is not None else origins.new_empty(0), fg, pg, fa, pa, *params)
        depth = depth.reshape(B, R)
        _depth_output(ctx, depth)
        return rgb.reshape(B, R, C - 1), depth

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g_rgb, g_depth):
        module, nat, opts = ctx.module, ctx.nat, ctx.opts
        _siren_autograd.check_same_weights(ctx, nat)
        B, R, N = ctx.dims
        origins, dirs, zc, rows, noise_f, fg, pg, fa, pa, *params = ctx.saved_tensors
        C = nat.C
        if ctx.depth_grad:
            g_rgb, g_depth = _upstream(ctx, g_rgb, g_depth, (B * R, C - 1))
            if g_rgb is None and g_depth is None:
                return (None,) * len(ctx.needs_input_grad)
        else:
            g_rgb, g_depth = g_rgb.contiguous().float().reshape(B * R, C - 1), None
        d = native.composite_backward(g_rgb, rows, zc, opts, noise=noise_f if noise_f.numel() else None, g_depth=g_depth)
        return _sparse_siren_backward(ctx, module, nat, ctx.needs_input_grad, B, R, N, 1, d, None, zc, None, origins, dirs, (fg, pg, fa, pa), params,
                                      [g for g in (g_rgb, g_depth) if g is not None])


class SparseSinglePassRenderDepthFunction(SparseSinglePassRenderFunction):
    """SparseSinglePassRenderFunction whose depth output carries the graph too."""
    depth_grad = True


# `siren.sparse_backward = "auto"`: the sparse node while it pays, the dense node otherwise.  What the sparse backward costs is set by the
# length of its buffers -- the forward's bound on the samples with a non-zero row, as a fraction of all samples -- and that number is on
# the host when the backward starts (no wait).  Model of the two steps at configs[1] (bench.py legs gstep / gstep_sparse):
# dense = forward-save + chain + weight gradients over everything; sparse = a no-grad render + the same over the fraction f, i.e.
# sparse / dense ~ 0.35 + 0.93 f: break-even at f ~ 0.7.  While the last observed fraction is above SPARSE_AUTO_MAX_FRACTION the dense node
# runs and every SPARSE_AUTO_PROBE_EVERY-th step is a sparse one that observes again (a probe at f = 1 costs + 28 % of one step).
SPARSE_AUTO_MAX_FRACTION = 0.6
SPARSE_AUTO_PROBE_EVERY = 50
# ... and only for renders of at least this many samples: the sparse step has about twice the dense step's fixed cost (more launches, the
# wait for the forward's bound), which short kernels do not pay back -- 4 x 32 x 32 x 12+12 (98,304 samples, 13 % kept): 2.37 against 2.17 ms;
# 6 x 64 x 64 x 12+12 (589,824, 21 % kept): 6.51 against 9.55 ms (tools/exp/gstep_small_shapes.py)
SPARSE_AUTO_MIN_SAMPLES = 262144


def plan_sparse_groups(caps, n_cus=256, group_cost=0.6):
    """caps[b]: slots image b needs (a multiple of 32).  -> [(images, cap)]: a partition of the batch into launch groups, each padded to its
    fullest image, that minimises  sum over groups of (rounds of 128-point workgroups over the CUs + group_cost)  -- the SIREN kernels are
    persistent, one workgroup per CU, so a group's time goes with ceil(images * cap / (128 * CUs)); group_cost (in rounds) stands for what a
    further group adds beside its kernels (five more launches, one more sum over the weight gradients).  Optimal over partitions of the
    images sorted by cap (dynamic programme, O(B^2)); ties go to fewer groups."""
    n = len(caps)
    order = sorted(range(n), key=lambda b: (-caps[b], b))
    unit = 128 * max(1, n_cus)
    best, cut = [0.0] + [float("inf")] * n, [0] * (n + 1)
    for j in range(1, n + 1):
        for i in range(j):
            c = best[i] + -(-((j - i) * caps[order[i]]) // unit) + group_cost
            if c < best[j] - 1e-9:
                best[j], cut[j] = c, i
    groups, j = [], n
    while j > 0:
        i = cut[j]
        groups.append((sorted(order[i:j]), caps[order[i]]))
        j = i
    return groups[::-1]


def _sparse_auto_state(module):
    st = module.__dict__.get("_sparse_auto")
    if st is None:
        st = module.__dict__["_sparse_auto"] = {"fraction": None, "dense_steps": 0, "last": None}
    return st


def sparse_auto_observe(module, fraction):
    """called by the sparse backward: the fraction of the samples its buffers were sized for"""
    _sparse_auto_state(module)["fraction"] = float(fraction)


def sparse_auto_choice(module, samples=None):
    """True: this step's render is the sparse node.  (Nothing observed yet: sparse -- that step is the first observation.)
    samples: samples of the render (all images, all passes); below SPARSE_AUTO_MIN_SAMPLES the dense node."""
    st = _sparse_auto_state(module)
    if samples is not None and samples < SPARSE_AUTO_MIN_SAMPLES:
        st["last"] = "dense"
        return False
    f = st["fraction"]
    if f is None or f <= SPARSE_AUTO_MAX_FRACTION:
        st["dense_steps"], st["last"] = 0, "sparse"
        return True
    st["dense_steps"] += 1
    if st["dense_steps"] >= SPARSE_AUTO_PROBE_EVERY:
        st["dense_steps"], st["last"] = 0, "probe"
        return True
    st["last"] = "dense"
    return False


# ----------------------------------------------------------------------------------------------------------------------------------
# The same render as TWO autograd nodes (round 4): for DistributedDataParallel.  With one node every gradient of the step becomes
# available at the same instant -- the end of the backward -- so DDP's bucketed all-reduce (124 MB, 113 MB of it the 96^3 feature
# grid; train_double_latent_semantic.py:148-150) can only start when there is nothing left to hide it under.  But the grid gradient is
# FINAL as soon as the last chain launch has scattered into it, with all the weight-gradient launches (a quarter of the step) still to
# run.  Split: the render stage's backward runs the composite backward and every chunk's chain, and returns the grid gradient; the
# engine hands it to the parameter (AccumulateGrad nodes run before any other ready node), DDP's hook starts the all-reduce of the
# grid's bucket on its communication stream, and only then the weight stage's backward runs the weight-gradient kernels over the dumps
# the chains left.  Price: the d(theta) dumps of all chunks are alive together (as large as the tape).  Opt-in per module
# (`siren.split_backward = True`, fenerf_amd.dist.prepare_for_ddp) -- DDP must also be allowed to reduce buckets in the order the
# gradients arrive (find_unused_parameters=False lets it rebuild its buckets after the first step; with the reference's
# find_unused_parameters=True the grid's bucket stays last in line and nothing overlaps).  What the render stage leaves for the weight
# stage lives for one backward pass only (an engine callback drops it): torch.autograd.grad on a subset of the inputs is supported in
# the sense that it returns what it can and leaks nothing; it does not deliver weight gradients unless the weight stage's inputs are asked for.
# ----------------------------------------------------------------------------------------------------------------------------------
# d(theta) dumps the render stage of a split backward leaves for the weight stage: the last SPLIT_KEEP_CHUNKS backward chunks' (a chunk = one
# pass of a 128 x 128 x 24 image = 4.4 GB at H = 256).  Two chunks = 3.6 ms of weight-gradient kernels for the 113-MB grid all-reduce to run
# beside (a ring all-reduce of that size over 8 GPUs' xGMI links is 1 - 2 ms), 8.8 GB instead of all 12 chunks' 52 GB at configs[2]'s
# 6-image micro-batch (round-4 review: peak 108 GB against 56.6 one-node; measured round 5: 76.1 GB with four chunks kept).
SPLIT_KEEP_CHUNKS = 2


class _SplitState:
    """what the render stage's backward leaves for the weight stage's backward of the same render"""
    def __init__(self):
        self.work = None


class HierarchicalWeightStage(torch.autograd.Function):
    """Upstream node: owns the raw FiLM parameters and every render weight EXCEPT the grid.  forward: a token; backward: the
    weight-gradient kernels over the dumps of the render stage."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, state, module, fg, pg, fa, pa, *params_no_grid):
        ctx.state, ctx.module = state, module
        return fg.new_zeros(1)

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, _g_token):
        w, ctx.state.work = ctx.state.work, None
        if w is None:
            raise RuntimeError("fenerf_amd: split backward: the render stage has not run (or ran twice) before the weight stage")
        module, nat, B = ctx.module, w["nat"], w["B"]
        need = ctx.needs_input_grad
        if w.get("abi"):        # fenerf_render_backward_stage(2): the kept chunks' weight gradients, the sums, the FiLM fold -- all in the library
            try:
                nat.set_grid_grad_mode(w["det"])     # the workspace's layout is stage 1's
                r = nat.render_backward_stage(2, w["keep"], B, w["R"], w["N"], w["save"], None, None, w["opts"], None, lock_view=w["lock_view"],
                                              tape_format=w["tape_format"], weights=w["weights"], chunk_points=w["chunk_points"], carry=w["carry"])
            finally:
                nat.release_split_workspace(w["carry"])
        else:
            r = _siren_autograd.run_weight_grads(nat, 2 * B, w["Pp"], w["film2"], w["pts2"], w["rd2"], w["out2"], w["d_out2"], w["tape2"], w["tape_e2"],
                                                 w["chunks"], w["dumps"], tape_format=w["tape_format"],
                                                 weights=_siren_autograd.film_layer_weights(module, w["params"]) if w["tape_format"] else None,
                                                 acc=w["acc"])
        params = w["params"]                                    # module._render_params() order, grid included
        grid = module._roles(params)["grid"]
        all_grads = _siren_autograd.assemble_param_grads(module, nat, params, r, None, None, [True] * len(params))
        no_grid = [g for p_, g in zip(params, all_grads) if p_ is not grid]
        # (the library's stage 2 has folded the two passes' FiLM rows already; the Python route's are folded here)
        return (None, None) + _siren_autograd.film_grads(r, need, 2, None if w.get("abi") else B) \
            + tuple(g if need[6 + i] else None for i, g in enumerate(no_grid))


class HierarchicalRenderSplitFunction(torch.autograd.Function):
    """Downstream node: the render itself.  Differentiable inputs: the weight stage's token and the grid.  backward: composite backward,
    every chunk's chain (with the fused grid scatter), the grid gradient; the dumps go to the weight stage through `state`."""
    depth_grad = False      # the two-node form has no depth variant (hierarchical_render_split refuses up front)

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, state, token, grid, module, opts, copts, lock_view, origins, dirs, z_c, u, noise_c, noise_f, fg, pg, fa, pa):
        ctx.state = state
        ctx.abi = USE_RENDER_ABI and not _siren_autograd.OVERLAP_WGRAD
        if not ctx.abi:
            return _hierarchical_forward(ctx, module, opts, copts, lock_view, origins, dirs, z_c, u, noise_c, noise_f, fg, pg, fa, pa, (),
                                         film_only=False)        # the split form exists for training steps: weight gradients are taken
        return _abi_forward(ctx, module, opts, lock_view, origins, dirs, z_c, u, noise_c, noise_f, fg, pg, fa, pa, (), film_only=False)

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g_rgb, _g_depth):
        module, nat, opts = ctx.module, ctx.nat, ctx.opts
        _siren_autograd.check_same_weights(ctx, nat)
        if ctx.abi:      # fenerf_render_backward_stage(1): composite backward, the early chunks whole, the kept chunks' chains, the grid gradient
            B, R, N = ctx.dims
            save, z_c, noise_f = ctx.saved_tensors
            keep = max(1, int(getattr(module, "split_keep_chunks", SPLIT_KEEP_CHUNKS)))
            params = module._render_params()
            weights = _siren_autograd.film_layer_weights(module, params) if ctx.tape_format else None
            det = _siren_autograd.deterministic_grid(module)
            nat.set_grid_grad_mode(det)
            g_grid, carry = nat.render_backward_stage(1, keep, B, R, N, save, z_c, noise_f if noise_f.numel() else None, opts, g_rgb.contiguous().float(),
                                                      lock_view=ctx.lock_view, tape_format=ctx.tape_format, weights=weights,
                                                      chunk_points=_siren_autograd.BACKWARD_CHUNK_POINTS)
            state = ctx.state
            state.work = dict(abi=True, det=det, nat=nat, B=B, R=R, N=N, save=save, opts=opts, lock_view=ctx.lock_view, tape_format=ctx.tape_format,
                              weights=weights, keep=keep, chunk_points=_siren_autograd.BACKWARD_CHUNK_POINTS, carry=carry, params=params)
            def drop():         # the engine has finished the pass: whatever the weight stage did not consume is dropped (see below)
                w_, state.work = state.work, None
                if w_ is not None:
                    nat.release_split_workspace(w_["carry"])
            torch.autograd.Variable._execution_engine.queue_callback(drop)
            g_token = torch.zeros(1, dtype=torch.float32, device=save.device) if ctx.needs_input_grad[1] else None
            if g_token is None:
                drop()
            return (None, g_token, g_grid if ctx.needs_input_grad[2] else None) + (None,) * 14
        B, R, N, P, Pp = ctx.dims
        pts2, rd, fg, pg, fa, pa, out2, tape2, tape_e2, z_f, zc, noise_f = ctx.saved_tensors
        d_out2, film2, rd2 = _python_composite_backward(nat, opts, ctx.dims, g_rgb, rd, (fg, pg, fa, pa), out2, z_f, zc, noise_f)
        chunks = _siren_autograd.plan_chunks(2 * B, Pp)
        # Bounded memory (round 5): only the LAST `split_keep_chunks` chunks' dumps are kept for the weight stage -- their weight-gradient
        # kernels are what the grid gradient's all-reduce runs beside; every earlier chunk takes its chain AND its weight gradients right
        # here, its dump freed before the next chain is launched (the one-node schedule), its gradients carried along as a running sum.
        # Same kernels on the same chunks, sums in chunk order: the gradients are those of the one-node backward.
        keep = max(1, int(getattr(module, "split_keep_chunks", SPLIT_KEEP_CHUNKS)))
        early, late = chunks[:max(0, len(chunks) - keep)], chunks[max(0, len(chunks) - keep):]
        tape_e = tape_e2 if tape_e2.numel() else None
        weights = _siren_autograd.film_layer_weights(module, module._render_params()) if ctx.tape_format else None
        acc, d_grid = _siren_autograd.GradSum(), None
        rows = _siren_autograd.begin_grid_gradient(module, nat, 2 * B * Pp)       # (this node exists for models with a grid)
        for c in early:
            d1, d_grid = _siren_autograd.run_chains(nat, 2 * B, Pp, film2, pts2, out2, d_out2, tape2, [c], tape_format=ctx.tape_format, d_grid=d_grid,
                                                    grid_rows=rows)
            _siren_autograd.run_weight_grads(nat, 2 * B, Pp, film2, pts2, rd2, out2, d_out2, tape2, tape_e, [c], d1, tape_format=ctx.tape_format,
                                             weights=weights, acc=acc, finish=False)
        dumps, d_grid = _siren_autograd.run_chains(nat, 2 * B, Pp, film2, pts2, out2, d_out2, tape2, late, tape_format=ctx.tape_format, d_grid=d_grid,
                                                   grid_rows=rows)
        if rows is not None:
            d_grid = rows.reduce(nat)
        state = ctx.state
        state.work = dict(nat=nat, B=B, Pp=Pp, film2=film2, pts2=pts2, rd2=rd2, out2=out2, d_out2=d_out2, tape2=tape2, tape_format=ctx.tape_format,
                          tape_e2=tape_e, chunks=late, dumps=dumps, acc=acc if early else None, params=module._render_params())
        # The dumps (as large as the tape) belong to THIS backward pass: if the weight stage does not consume them -- torch.autograd.grad
        # with only the grid as input, an exception between the two stages -- they are dropped when the engine finishes the pass, not
        # when the graph dies; a retained graph's next backward then starts from a clean state instead of overwriting a stale one.
        torch.autograd.Variable._execution_engine.queue_callback(lambda: setattr(state, "work", None))
        g_grid = nat.grid_gradient_ncdhw(d_grid).contiguous() if ctx.needs_input_grad[2] else None
        g_token = torch.zeros(1, dtype=torch.float32, device=out2.device) if ctx.needs_input_grad[1] else None
        if g_token is None:
            ctx.state.work = None          # nothing upstream will consume the dumps
        return (None, g_token, g_grid) + (None,) * 14


def hierarchical_render_split(module, opts, copts, lock_view, origins, dirs, z_c, u, noise_c, noise_f, fg, pg, fa, pa, depth_grad=False):
    """The two-node form of HierarchicalRenderFunction.apply(...) for a module with a feature grid (see the banner above)."""
    if depth_grad:
        raise NotImplementedError("fenerf_amd: the two-node (split_backward) render has no differentiable depth (fenerf_render_backward_stage "
                                  "takes no depth gradient); set siren.split_backward = False")
    params = module._render_params()
    grid = module._roles(params)["grid"]
    state = _SplitState()
    token = HierarchicalWeightStage.apply(state, module, fg, pg, fa, pa, *[p_ for p_ in params if p_ is not grid])
    return HierarchicalRenderSplitFunction.apply(state, token, grid, module, opts, copts, lock_view, origins, dirs, z_c, u, noise_c, noise_f,
                                                 fg.detach(), pg.detach(), fa.detach(), pa.detach())
