"""SIREN radiance-field heads -- drop-in for the reference's siren/siren.py classes that are reachable from
its curriculums.  The nn.Module only OWNS the parameters (same attribute / state_dict names as the reference,
so pickled reference checkpoints load after fenerf_amd.compat.install_aliases()); evaluation is a single
fused HIP kernel behind fenerf_siren_forward (include/fenerf.h).  The mapping networks (z -> FiLM
frequencies / phases; per image, tiny) stay in PyTorch.

reference: FiLMLayer siren.py:113-123, CustomMappingNetwork :82-102, frequency_init :104-110,
UniformBoxWarp :181-187, SPATIALSIRENBASELINE :189-244, SIRENBASELINESEMANTICDISENTANGLE :1163-1229,
TextureEmbeddingPiGAN128SEMANTICDISENTANGLE :1451-1530 (+256 :1533, _DIM_96 :1541).
"""
import numpy as np
import torch
import torch.nn as nn

from .. import native
from . import autograd as _autograd


def kaiming_leaky_init(m):
    if m.__class__.__name__.find("Linear") != -1:
        torch.nn.init.kaiming_normal_(m.weight, a=0.2, mode="fan_in", nonlinearity="leaky_relu")


def frequency_init(freq):
    def init(m):
        with torch.no_grad():
            if isinstance(m, nn.Linear):
                num_input = m.weight.size(-1)
                m.weight.uniform_(-np.sqrt(6 / num_input) / freq, np.sqrt(6 / num_input) / freq)
    return init


def first_layer_film_sine_init(m):
    with torch.no_grad():
        if isinstance(m, nn.Linear):
            num_input = m.weight.size(-1)
            m.weight.uniform_(-1 / num_input, 1 / num_input)


def modified_first_sine_init(m):
    with torch.no_grad():
        if isinstance(m, nn.Linear):
            m.weight.uniform_(-1 / 3, 1 / 3)


class CustomMappingNetwork(nn.Module):
    """z -> (frequencies, phase_shifts); stays PyTorch (siren.py:82-102)."""

    def __init__(self, z_dim, map_hidden_dim, map_output_dim, n_blocks=3):
        super().__init__()
        layers = [nn.Linear(z_dim, map_hidden_dim), nn.LeakyReLU(0.2, inplace=True)]
        for _ in range(n_blocks):
            layers += [nn.Linear(map_hidden_dim, map_hidden_dim), nn.LeakyReLU(0.2, inplace=True)]
        layers.append(nn.Linear(map_hidden_dim, map_output_dim))
        self.network = nn.Sequential(*layers)
        self.network.apply(kaiming_leaky_init)
        with torch.no_grad():
            self.network[-1].weight *= 0.25

    # batches up to this size run as fenerf_mapping_forward / _backward (one launch forward, three backward, instead of ~9 and ~30 ATen
    # launches of 5 us each); larger ones -- the 10,000 latents of generate_avg_frequencies -- are rocBLAS GEMMs in PyTorch
    NATIVE_MAX_BATCH = 64

    def _native_ok(self, z):
        return (z.is_cuda and z.dim() == 2 and 0 < z.shape[0] <= self.NATIVE_MAX_BATCH and not z.requires_grad
                and self.network[0].out_features <= 1024 and z.shape[1] <= 4096 and len(self.network) // 2 + 1 <= 8)

    def forward(self, z):
        if self._native_ok(z):
            linears = [m for m in self.network if isinstance(m, nn.Linear)]
            return _MappingFunction.apply(z, len(linears), *[l.weight for l in linears], *[l.bias for l in linears])
        out = self.network(z)
        half = out.shape[-1] // 2
        return out[..., :half], out[..., half:]


class _MappingFunction(torch.autograd.Function):
    """CustomMappingNetwork on the native kernels (fenerf_mapping.hip): forward = one launch, backward = three; gradients wrt every
    weight and bias (z takes none: the reference samples its latents)."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, z, n, *params):
        weights, biases = list(params[:n]), list(params[n:])
        out, acts = native.mapping_forward(weights, biases, z)
        ctx.n = n
        ctx.save_for_backward(z, acts, *params)
        # the two halves as the Function's OWN outputs: left to autograd, the backward of the two slices of `out` is two zero fills, two
        # strided copies and an add (5 launches per network per step) before this backward even starts; here it is one concatenation
        # (fresh tensors, not two views of `out`: autograd refuses in-place edits -- frequencies.mul_(...) -- of a Function's view outputs,
        # which the reference's plain slices allow)
        half = out.shape[-1] // 2
        return out[..., :half].clone(), out[..., half:].clone()

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, d_freq, d_phase):
        z, acts, *params = ctx.saved_tensors
        n = ctx.n
        dW, db = native.mapping_backward(list(params[:n]), list(params[n:]), z, acts, torch.cat([d_freq.float(), d_phase.float()], -1))
        need = ctx.needs_input_grad[2:]
        return (None, None) + tuple(g if need[i] else None for i, g in enumerate(dW + db))


class FiLMLayer(nn.Module):
    """Parameter holder for one FiLM layer (the sin(freq*(Wx+b)+phase) itself runs fused on the GPU)."""

    def __init__(self, input_dim, hidden_dim):
        super().__init__()
        self.layer = nn.Linear(input_dim, hidden_dim)


class UniformBoxWarp(nn.Module):
    def __init__(self, sidelength):
        super().__init__()
        self.scale_factor = 2 / sidelength

    def forward(self, coordinates):
        return coordinates * self.scale_factor


class _NativeSiren(nn.Module):
    """Shared machinery: exports parameters to the native model, re-packs when they change."""

    KIND = None
    N_LABEL_LAYERS = 0
    GRID_CH = 0
    # "f16x3": error-compensated fp16 MFMA (3 MFMAs per product, fp32 accumulate) -- measured accuracy equal to the exact
    # kernel (rgb 3e-7 vs reference) and ~2.7x faster; "f32": exact fp32 MFMA (bitwise an fmaf chain).
    precision = "f16x3"
    # Weight-gradient operands of the differentiable path: "f32" (default) = fp32-class gradients everywhere; "amp" = in backward
    # chunks of >= AMP_MIN_POINTS points the chain kernel hands d theta and the layer inputs to the weight-gradient kernel as bf16 (one
    # MFMA per product, fp32 accumulate) -- unbiased, ~1e-3 of a gradient entry's per-point noise floor: the class of the reference's
    # own autocast training loop (train_double_latent_semantic.py:402-446), 13 % less step time.  Never the default.
    # "tape16" (round 5, f16x3 models) = fp32-class operands, but the tape between forward and backward holds frac(theta) as 16-bit fixed
    # point instead of the fp32 accumulators (include/fenerf.h FENERF_TAPE_U16): half the tape bytes in three kernels, +-4.8e-5 rad on
    # every recomputed activation, gradients within ~1.2e-4 of fp64 autograd instead of ~4e-5 -- a tier between the two.  Applies to
    # backward passes that take weight gradients; inversion (FiLM gradients only) keeps the fp32 tape whatever this says.
    # "amp16" = both: bf16 weight-gradient operands AND the 16-bit tape (the FiLM frequency gradients, which "amp" takes from the fp32 tape,
    # then come from the bf16 products too: everything AMP class) -- the fastest generator step this package has.
    grad_precision = "f32"
    AMP_MIN_POINTS = 65536
    FREQ_FROM_WGRAD = True      # (round 5; False = rounds 2-4: the chain kernel forms sum_p d theta * tape itself -- kept for A/B runs and tests)
    # Gradient wrt the feature grid (spatial_embeddings) of the differentiable path: None (default) follows torch.use_deterministic_algorithms
    # at the time the backward runs -- on: every row's d(grid features) is kept and all rows are reduced once in exact int64 arithmetic
    # (include/fenerf.h FENERF_GRID_GRAD_DETERMINISTIC: the same bits run to run, for any chunking, one- or two-node, dense or sparse); off:
    # the chain kernels' fp32 atomics (faster; the last bits vary).  True / False force one of the two (False under torch's switch raises,
    # as torch does for an operation without a deterministic form).
    deterministic_backward = None

    def tape_format(self, nat, film_only):
        """the tape format (_lib.TAPE_*) a differentiable evaluation on `nat` uses"""
        from .. import _lib
        if nat.precision != "f16x3" or film_only:
            return _lib.TAPE_F32
        if self.grad_precision in ("tape16", "amp16"):
            return _lib.TAPE_U16
        # default precision: the fp32 tape; the FiLM frequency gradients come from the weight-gradient sums (FENERF_TAPE_F32_W: the chain kernel
        # then skips its second FiLM sum, a fifth of its VALU instructions) unless FREQ_FROM_WGRAD is off.  "amp" keeps the chain's own sums:
        # its frequency gradients stay fp32 class while the weight gradients' operands are bf16.
        return _lib.TAPE_F32_W if (self.FREQ_FROM_WGRAD and self.grad_precision == "f32") else _lib.TAPE_F32

    def _spec(self):
        H = self.hidden_dim
        n_color = 1 if self.KIND == "spatial" else len(self.color_layer_sine)
        return dict(kind=self.KIND, hidden_dim=H, n_geo=len(self.network), n_color=n_color, grid_ch=self.GRID_CH,
                    n_label_layers=self.N_LABEL_LAYERS, output_dim=self.output_dim)

    @staticmethod
    def _is_render_param(name):
        """parameters the native SIREN kernels consume: everything but the mapping networks and (SPATIALSIRENGRID) the latent-grid
        generator, which run in PyTorch per image"""
        return "mapping_network" not in name and not name.startswith("grid_latent_network")

    def _named_render_params(self):
        return [(n, p) for n, p in self.named_parameters() if self._is_render_param(n)]

    def _render_params(self):
        return [p for _, p in self._named_render_params()]

    def _state_numpy(self):
        return {n: p.detach().to("cpu", torch.float32).contiguous().numpy() for n, p in self._named_render_params()}

    def native(self, device=None):
        """The FenerfModel for the current parameter values on `device` (re-packed lazily after updates)."""
        params = self._render_params()
        device = torch.device(device if device is not None else params[0].device)
        ver = tuple(p._version for p in params) + tuple(p.data_ptr() for p in params)
        nat = self.__dict__.get("_native_model")
        if nat is None or nat.device != device or nat.requested_precision != self.precision:      # ("f16x2" / "f16x3c2": f16x3 handles with a reduced-precision forward)
            nat = native.NativeModel(self._state_numpy(), self._spec(), device, self.precision)
            self.__dict__["_native_model"] = nat
        elif self.__dict__.get("_native_version") != ver:
            if params[0].is_cuda:      # weights already live on the GPU (training): re-pack there, not through the host
                nat.load_from_device(dict(self._named_render_params()),
                                     maybe_unchanged=self.__dict__.get("_native_packed") == ver)
            else:
                nat.update(self._state_numpy())
        self.__dict__["_native_version"] = self.__dict__["_native_packed"] = ver
        return nat

    def native_differentiable(self, device=None):
        """The FenerfModel (same precision as the no-grad path) with the backward-chain stream resident (generator step /
        inversion); re-packed lazily, on the device."""
        params = self._render_params()
        device = torch.device(device if device is not None else params[0].device)
        ver = tuple(p._version for p in params) + tuple(p.data_ptr() for p in params)
        nat = self.__dict__.get("_native_diff")
        base = "f16x3" if self.precision in native.NativeModel.FORWARD_MODES else self.precision     # the differentiable path always runs three terms
        amp = self.AMP_MIN_POINTS if (self.grad_precision in ("amp", "amp16") and base == "f16x3") else 0
        if nat is None or nat.device != device or nat.precision != base or nat.wgrad_bf16_min_points != amp:
            nat = native.NativeModel(self._state_numpy(), self._spec(), device, base, differentiable=True,
                                     wgrad_bf16_min_points=amp)
            self.__dict__["_native_diff"] = nat
        elif self.__dict__.get("_native_diff_version") != ver:
            # weights live on the GPU during training: re-pack there (a gather), never through the host.  Same version counters as
            # at the last pack = a forced invalidation (mode switch, invalidate_native()): the content is compared first, so that a
            # train() / eval() round trip between a forward and its backward does not make the backward refuse (pack_generation)
            nat.load_from_device(dict(self._named_render_params()),
                                 maybe_unchanged=self.__dict__.get("_native_diff_packed") == ver)
        self.__dict__["_native_diff_version"] = self.__dict__["_native_diff_packed"] = ver
        return nat

    def invalidate_native(self):
        """Force a re-pack of the native models at the next render.  Parameter changes are normally detected through the
        tensors' version counters; writes through `param.data` (torch_ema's copy_to / restore do that) bypass them."""
        self.__dict__.pop("_native_version", None)
        self.__dict__.pop("_native_diff_version", None)

    def train(self, mode=True):
        # The reference brackets every EMA swap with generator.eval() / generator.train() (train_double_latent_semantic.py:
        # 487-489, :522 -> :267), and torch_ema writes through param.data, which no version counter sees: treat a mode switch
        # as "weights may have changed".
        self.invalidate_native()
        return super().train(mode)

    def _roles(self, params):
        """`params` = tensors in _render_params() order -> which layer each one is."""
        names = [n for n, _ in self._named_render_params()]
        t = dict(zip(names, params))
        n_geo = len(self.network)
        if self.KIND == "spatial":
            color = [(t["color_layer_sine.layer.weight"], t["color_layer_sine.layer.bias"])]
        else:
            color = [(t[f"color_layer_sine.{i}.layer.weight"], t[f"color_layer_sine.{i}.layer.bias"]) for i in range(len(self.color_layer_sine))]
        return dict(geo=[(t[f"network.{i}.layer.weight"], t[f"network.{i}.layer.bias"]) for i in range(n_geo)], color=color,
                    label=[(t[f"label_layer_linear.{i}.weight"], t[f"label_layer_linear.{i}.bias"]) for i in range(self.N_LABEL_LAYERS)],
                    sigma=(t["final_layer.weight"], t["final_layer.bias"]),
                    rgb=(t["color_layer_linear.0.weight"], t["color_layer_linear.0.bias"]), grid=t.get("spatial_embeddings"))

    def _wants_grad(self, *tensors):
        return torch.is_grad_enabled() and (any(t is not None and t.requires_grad for t in tensors) or
                                            any(p.requires_grad for p in self._render_params()))

    def __getstate__(self):
        st = self.__dict__.copy()
        for k in ("_native_model", "_native_version", "_native_packed", "_native_diff", "_native_diff_version", "_native_diff_packed"):
            st.pop(k, None)
        return st


class _DoubleLatentSiren(_NativeSiren):
    def forward(self, input, z_geo, z_app, ray_directions, **kwargs):
        fg, pg = self.geo_mapping_network(z_geo)
        fa, pa = self.app_mapping_network(z_app)
        return self.forward_with_frequencies_phase_shifts(input, fg, fa, pg, pa, ray_directions, **kwargs)

    def forward_with_frequencies_phase_shifts(self, input, frequencies_geo, frequencies_app, phase_shifts_geo,
                                              phase_shifts_app, ray_directions, **kwargs):
        """[B,P,3] points, [B,P,3] dirs -> [B,P,output_dim] = [labels | rgb | sigma]   (siren.py:1509-1530)"""
        if self._wants_grad(input, ray_directions, frequencies_geo, frequencies_app, phase_shifts_geo, phase_shifts_app):
            return _autograd.siren_apply(self, input, ray_directions, frequencies_geo, phase_shifts_geo, frequencies_app,
                                         phase_shifts_app)
        return self.native(input.device).siren_forward(input, ray_directions, frequencies_geo, phase_shifts_geo,
                                                       frequencies_app, phase_shifts_app)

    def geometry(self, input, z_geo, **kwargs):
        """[B,P,3] points -> [B,P,n_lab+1] = [labels | sigma]: what forward() returns in those channels.  They depend on the geometry
        latent alone (siren.py:1514, :1522-1527), so no z_app and no view direction is taken."""
        fg, pg = self.geo_mapping_network(z_geo)
        return self.geometry_with_frequencies_phase_shifts(input, fg, pg, **kwargs)

    def geometry_with_frequencies_phase_shifts(self, input, frequencies_geo, phase_shifts_geo, **kwargs):
        """Without grad, on a model the density route serves (NativeModel.supports_density), the native labels + sigma query: the bits of
        forward_with_frequencies_phase_shifts' channels without its colour branch.  Otherwise that forward, sliced (the colour inputs it
        needs are zeros and the locked view direction: labels and sigma do not read them) -- differentiable wherever the module is."""
        if not self._wants_grad(input, frequencies_geo, phase_shifts_geo):
            nat = self.native(input.device)
            if nat.supports_density():
                return nat.siren_density(input, frequencies_geo, phase_shifts_geo, labels=True)
        n_app = len(self.color_layer_sine) * self.hidden_dim
        zeros = frequencies_geo.new_zeros((frequencies_geo.shape[0], n_app))
        rd = torch.zeros_like(input)
        rd[..., -1] = -1
        out = self.forward_with_frequencies_phase_shifts(input, frequencies_geo, zeros, phase_shifts_geo, zeros, rd)
        return torch.cat([out[..., :-4], out[..., -1:]], dim=-1)


class SIRENBASELINESEMANTICDISENTANGLE(_DoubleLatentSiren):
    """README 'w/o latent grid' model (siren.py:1163-1229)."""
    KIND, N_LABEL_LAYERS, GRID_CH = "baseline", 2, 0

    def __init__(self, input_dim=2, z_geo_dim=100, z_app_dim=100, hidden_dim=256, output_dim=1, device=None):
        super().__init__()
        self.device, self.input_dim, self.z_geo_dim, self.z_app_dim = device, input_dim, z_geo_dim, z_app_dim
        self.hidden_dim, self.output_dim = hidden_dim, output_dim
        self.network = nn.ModuleList([FiLMLayer(3, hidden_dim)] + [FiLMLayer(hidden_dim, hidden_dim) for _ in range(7)])
        self.final_layer = nn.Linear(hidden_dim, 1)
        self.color_layer_sine = nn.ModuleList([FiLMLayer(hidden_dim + 3, hidden_dim), FiLMLayer(hidden_dim, hidden_dim),
                                               FiLMLayer(hidden_dim, hidden_dim)])
        self.color_layer_linear = nn.Sequential(nn.Linear(hidden_dim, 3))
        self.geo_mapping_network = CustomMappingNetwork(z_geo_dim, 256, len(self.network) * hidden_dim * 2)
        self.app_mapping_network = CustomMappingNetwork(z_app_dim, 256, len(self.color_layer_sine) * hidden_dim * 2)
        self.label_layer_linear = nn.Sequential(nn.Linear(hidden_dim, hidden_dim), nn.Linear(hidden_dim, self.output_dim - 4))
        for mod in (self.network, self.final_layer, self.color_layer_sine, self.color_layer_linear, self.label_layer_linear):
            mod.apply(frequency_init(25))
        self.network[0].apply(first_layer_film_sine_init)
        self.gridwarper = UniformBoxWarp(0.24)


class TextureEmbeddingPiGAN128SEMANTICDISENTANGLE(_DoubleLatentSiren):
    """FENeRF 'w/ latent grid' model: 32-channel 3-D feature grid feeding the colour branch (siren.py:1451-1530)."""
    KIND, N_LABEL_LAYERS, GRID_CH = "texture", 3, 32

    def __init__(self, input_dim=2, z_geo_dim=100, z_app_dim=100, hidden_dim=128, output_dim=1, device=None):
        super().__init__()
        self.device, self.input_dim, self.z_geo_dim, self.z_app_dim = device, input_dim, z_geo_dim, z_app_dim
        self.hidden_dim, self.output_dim = hidden_dim, output_dim
        self.network = nn.ModuleList([FiLMLayer(3, hidden_dim)] + [FiLMLayer(hidden_dim, hidden_dim) for _ in range(7)])
        self.final_layer = nn.Linear(hidden_dim, 1)
        self.color_layer_sine = nn.ModuleList([FiLMLayer(hidden_dim + 32 + 3, hidden_dim), FiLMLayer(hidden_dim, hidden_dim),
                                               FiLMLayer(hidden_dim, hidden_dim)])
        self.color_layer_linear = nn.Sequential(nn.Linear(hidden_dim, 3))
        self.geo_mapping_network = CustomMappingNetwork(z_geo_dim, 256, len(self.network) * hidden_dim * 2)
        self.app_mapping_network = CustomMappingNetwork(z_app_dim, 256, len(self.color_layer_sine) * hidden_dim * 2)
        self.label_layer_linear = nn.Sequential(nn.Linear(hidden_dim, hidden_dim), nn.Linear(hidden_dim, hidden_dim),
                                                nn.Linear(hidden_dim, self.output_dim - 4))
        for mod in (self.network, self.final_layer, self.color_layer_sine, self.color_layer_linear, self.label_layer_linear):
            mod.apply(frequency_init(25))
        self.network[0].apply(modified_first_sine_init)
        self.spatial_embeddings = nn.Parameter(torch.randn(1, 32, 96, 96, 96) * 0.01)
        self.gridwarper = UniformBoxWarp(0.24)


class TextureEmbeddingPiGAN256SEMANTICDISENTANGLE(TextureEmbeddingPiGAN128SEMANTICDISENTANGLE):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs, hidden_dim=256)
        self.spatial_embeddings = nn.Parameter(torch.randn(1, 32, 64, 64, 64) * 0.1)


class TextureEmbeddingPiGAN256SEMANTICDISENTANGLE_DIM_96(TextureEmbeddingPiGAN128SEMANTICDISENTANGLE):
    """The model of curriculum CelebA_double_semantic_texture_embedding_256_dim_96 (curriculums.py:159): H=256, 96^3 grid."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs, hidden_dim=256)
        self.spatial_embeddings = nn.Parameter(torch.randn(1, 32, 96, 96, 96) * 0.1)


class SPATIALSIRENBASELINE(_NativeSiren):
    """Single-latent pi-GAN head, rgb+sigma (siren.py:189-244); curriculum `CelebA`."""
    KIND, N_LABEL_LAYERS, GRID_CH = "spatial", 0, 0

    def __init__(self, input_dim=2, z_dim=100, hidden_dim=256, output_dim=1, device=None):
        super().__init__()
        self.device, self.input_dim, self.z_dim = device, input_dim, z_dim
        self.hidden_dim = hidden_dim
        self.output_dim = 4  # the reference stores output_dim but always emits [rgb | sigma] (siren.py:244)
        self.network = nn.ModuleList([FiLMLayer(3, hidden_dim)] + [FiLMLayer(hidden_dim, hidden_dim) for _ in range(7)])
        self.final_layer = nn.Linear(hidden_dim, 1)
        self.color_layer_sine = FiLMLayer(hidden_dim + 3, hidden_dim)
        self.color_layer_linear = nn.Sequential(nn.Linear(hidden_dim, 3))
        self.mapping_network = CustomMappingNetwork(z_dim, 256, (len(self.network) + 1) * hidden_dim * 2)
        for mod in (self.network, self.final_layer, self.color_layer_sine, self.color_layer_linear):
            mod.apply(frequency_init(25))
        self.network[0].apply(first_layer_film_sine_init)
        self.gridwarper = UniformBoxWarp(0.24)

    def forward(self, input, z, ray_directions, **kwargs):
        frequencies, phase_shifts = self.mapping_network(z)
        return self.forward_with_frequencies_phase_shifts(input, frequencies, phase_shifts, ray_directions, **kwargs)

    def split_film(self, frequencies, phase_shifts):
        """[B, 9H] -> geo [B, 8H] + colour [B, H] (the last H, siren.py:241)."""
        H = self.hidden_dim
        n = len(self.network) * H
        return (frequencies[..., :n].contiguous(), phase_shifts[..., :n].contiguous(),
                frequencies[..., -H:].contiguous(), phase_shifts[..., -H:].contiguous())

    def forward_with_frequencies_phase_shifts(self, input, frequencies, phase_shifts, ray_directions, **kwargs):
        fg, pg, fa, pa = self.split_film(frequencies, phase_shifts)
        if self._wants_grad(input, ray_directions, frequencies, phase_shifts):
            return _autograd.siren_apply(self, input, ray_directions, fg, pg, fa, pa)
        return self.native(input.device).siren_forward(input, ray_directions, fg, pg, fa, pa)


class SPATIALSIRENGRID(SPATIALSIRENBASELINE):
    """SPATIALSIRENBASELINE whose FiLM parameters are PER SAMPLE POINT (siren.py:413-518): a 2-D grid of local latents
    (32 channels, from the StyleGAN2-style `grid_latent_network`, siren/latent_grid.py -> fenerf_amd/siren/latent_grid.py) is sampled
    bilinearly at every point's (x, z), a one-block mapping network turns the 32-d local latent into that point's frequencies / phase
    shifts, and the SIREN is evaluated in local cell coordinates.
    forward(input, z, ray_directions) is the reference's: latent grid (PyTorch, once per image) -> local latents and local
    coordinates (torch statements of :479-518, 128 B per point) -> ONE native launch that evaluates the per-point mapping network AND
    the FiLM-SIREN (fenerf_siren_forward_local: the 18 KB of FiLM parameters per point never exist in memory).
    forward_with_frequencies_phase_shifts with explicit per-point [B, P, 9H] parameters (the reference's signature, :464) runs
    fenerf_siren_forward_pointwise on the caller's tensors.  Both are exact-fp32 kernels whatever `precision` says -- fp32-class
    results is what "f16x3" promises too.
    Under autograd (an input, latent or parameter requires grad in grad mode) the module is what the reference's is: an ordinary
    differentiable nn.Module.  Since round 6 the per-point-modulated SIREN itself is native there too (`siren.autograd.
    PointwiseSirenFunction` over fenerf_siren_forward_save_pointwise / _backward_pointwise / _param_grads_pointwise: exact-fp32 forward
    with tape, chain kernel reading every lane's own FiLM block, weight-gradient jobs that scale d(theta) by the POINT's frequency while
    staging it -- the per-image path's sum_images diag(f_image) sum_points d(theta) x^T does not exist with per-point frequencies -- and
    the gradients wrt the per-point frequencies / phase shifts as [B, P, 9H] tensors).  The per-point mapping network (two nn.Linear on
    [B*P, 32] / [B*P, 256]: plain rocBLAS GEMMs), the bilinear latent sampling and StyleGenerator2D stay PyTorch-ROCm autograd, through which
    the gradient reaches the latent grid and z.  `NATIVE_POINTWISE_BACKWARD = False` (or sample positions / view directions that require
    grad) takes the rounds-3-5 route: the SIREN as PyTorch-ROCm ops (`_film_siren_torch`), kept as the A/B reference of the tests.  The
    variant is in no curriculum and the reference never trains it; pinned to the reference module's own autograd
    (tiny_spatial_grid.npz)."""
    NATIVE_POINTWISE_BACKWARD = True

    def __init__(self, input_dim=2, z_dim=100, hidden_dim=256, output_dim=1, device=None):
        super().__init__(input_dim=input_dim, z_dim=z_dim, hidden_dim=hidden_dim, output_dim=output_dim, device=device)
        from .latent_grid import StyleGenerator2D
        self.local_coordinates = True
        self.mapping_network = CustomMappingNetwork(32, 256, (len(self.network) + 1) * hidden_dim * 2, n_blocks=1)   # :440
        self.grid_latent_network = StyleGenerator2D(out_res=32, out_ch=32, z_dim=z_dim, ch_mul=1, ch_max=256, skip_conn=False)   # :442

    def forward(self, input, z, ray_directions, **kwargs):
        return self.forward_with_latent_grid(input, self.grid_latent_network(z), ray_directions, **kwargs)   # :453

    def forward_with_latent_grid(self, input, latent_grid, ray_directions, **kwargs):
        """The body of the reference's forward after `latent_grid = self.grid_latent_network(z)` (siren.py:453-463)."""
        input_grid = self.gridwarper(input)
        sampled_latent = self.sample_local_latents(latent_grid, input_grid)
        if self.local_coordinates:
            input = self.get_local_coordinates(global_coords=input, local_grid_length=32, preserve_y=False)
        if self._wants_grad(input, ray_directions, sampled_latent, *self.mapping_network.parameters()):
            frequencies, phase_shifts = self.mapping_network(sampled_latent)
            return self._film_siren_grad(input, frequencies, phase_shifts, ray_directions)
        return self.native_local(input.device).forward(input, ray_directions, sampled_latent)

    def _film_siren_grad(self, input, frequencies, phase_shifts, ray_directions):
        """the per-point-modulated SIREN under autograd: native (PointwiseSirenFunction) unless switched off or a gradient wrt the sample
        positions / view directions is wanted (not provided natively, as everywhere in this package)"""
        wants_xyz = input.requires_grad or (ray_directions is not None and ray_directions.requires_grad)
        if not self.NATIVE_POINTWISE_BACKWARD or wants_xyz or frequencies.dim() != 3 or input.device.type != "cuda":
            return self._film_siren_torch(input, frequencies, phase_shifts, ray_directions)
        fg, pg, fa, pa = self.split_film(frequencies, phase_shifts)
        return _autograd.siren_apply_pointwise(self, input, ray_directions, fg, pg, fa, pa)

    def native_pointwise_differentiable(self, device=None):
        """The exact-fp32 FenerfModel with the backward stream resident (fenerf_siren_*_pointwise), re-packed lazily on the device."""
        params = self._render_params()
        device = torch.device(device if device is not None else params[0].device)
        ver = tuple(p._version for p in params) + tuple(p.data_ptr() for p in params)
        nat = self.__dict__.get("_native_pw_diff")
        if nat is None or nat.device != device:
            nat = native.NativeModel(self._state_numpy(), self._spec(), device, "f32", differentiable=True)
            self.__dict__["_native_pw_diff"] = nat
        elif self.__dict__.get("_native_pw_diff_version") != ver:
            nat.load_from_device(dict(self._named_render_params()), maybe_unchanged=self.__dict__.get("_native_pw_diff_packed") == ver)
        self.__dict__["_native_pw_diff_version"] = self.__dict__["_native_pw_diff_packed"] = ver
        return nat

    def _film_siren_torch(self, input, frequencies, phase_shifts, ray_directions):
        """siren.py:464-477 as differentiable PyTorch-ROCm ops (per-point [B, P, 9H] or per-image [B, 9H] FiLM blocks): the autograd
        route of this variant -- see the class docstring for why it is not the native chain."""
        if input.device.type != "cuda":
            raise RuntimeError("fenerf_amd renders on the GPU only (there is no CPU path); got device %s" % input.device)
        H = self.hidden_dim
        if frequencies.dim() == 2:
            frequencies, phase_shifts = frequencies[:, None, :], phase_shifts[:, None, :]
        frequencies = frequencies * 15 + 30
        x = self.gridwarper(input)
        for i, layer in enumerate(self.network):
            x = torch.sin(frequencies[..., i * H:(i + 1) * H] * layer.layer(x) + phase_shifts[..., i * H:(i + 1) * H])
        sigma = self.final_layer(x)
        c = torch.sin(frequencies[..., -H:] * self.color_layer_sine.layer(torch.cat([ray_directions, x], dim=-1)) + phase_shifts[..., -H:])
        return torch.cat([torch.sigmoid(self.color_layer_linear(c)), sigma], dim=-1)

    def native_local(self, device=None):
        """The FenerfLocalModel (SIREN + per-point mapping network in one packed fp32 stream) for the current parameter values."""
        params = [p for n, p in self.named_parameters() if not n.startswith("grid_latent_network")]
        device = torch.device(device if device is not None else params[0].device)
        ver = tuple(p._version for p in params) + tuple(p.data_ptr() for p in params)
        nat = self.__dict__.get("_native_local")
        if nat is None or nat.device != device or self.__dict__.get("_native_local_version") != ver:
            if nat is not None:
                nat.close()
            mp = {n[len("mapping_network.network."):]: p.detach().to("cpu", torch.float32).contiguous().numpy()
                  for n, p in self.named_parameters() if n.startswith("mapping_network.network.")}
            nat = native.NativeLocalModel(self._state_numpy(), self._spec(), mp, device)
            self.__dict__["_native_local"] = nat
            self.__dict__["_native_local_version"] = ver
        return nat

    def native(self, device=None):
        """explicit per-point FiLM tensors run on the exact-fp32 kernel (fenerf_siren_forward_pointwise)"""
        params = self._render_params()
        device = torch.device(device if device is not None else params[0].device)
        ver = tuple(p._version for p in params) + tuple(p.data_ptr() for p in params)
        nat = self.__dict__.get("_native_pw")
        if nat is None or nat.device != device:
            nat = native.NativeModel(self._state_numpy(), self._spec(), device, "f32")
            self.__dict__["_native_pw"] = nat
        elif self.__dict__.get("_native_pw_version") != ver:
            nat.update(self._state_numpy())
        self.__dict__["_native_pw_version"] = ver
        return nat

    def invalidate_native(self):
        super().invalidate_native()
        self.__dict__.pop("_native_local_version", None)
        self.__dict__.pop("_native_pw_version", None)
        self.__dict__.pop("_native_pw_diff_version", None)

    def __getstate__(self):
        st = super().__getstate__()
        for k in ("_native_local", "_native_local_version", "_native_pw", "_native_pw_version", "_native_pw_diff", "_native_pw_diff_version",
                  "_native_pw_diff_packed"):
            st.pop(k, None)
        return st

    def forward_with_frequencies_phase_shifts(self, input, frequencies, phase_shifts, ray_directions, **kwargs):
        """frequencies / phase_shifts [B, P, 9H]: one FiLM block per point (siren.py:464-477); [B, 9H] behaves like the parent."""
        if frequencies.dim() == 2:
            return super().forward_with_frequencies_phase_shifts(input, frequencies, phase_shifts, ray_directions, **kwargs)
        if self._wants_grad(input, ray_directions, frequencies, phase_shifts):
            return self._film_siren_grad(input, frequencies, phase_shifts, ray_directions)
        fg, pg, fa, pa = self.split_film(frequencies, phase_shifts)
        return self.native(input.device).siren_forward_pointwise(input, ray_directions, fg, pg, fa, pa)

    @staticmethod
    def sample_local_latents(local_latents, xyz):
        """[B, 32, h, w] latents sampled bilinearly (align_corners=False, zeros padding) at every point's (x, z) -> [B, P, 32]
        (siren.py:479-499)."""
        B, local_z_dim, _, _ = local_latents.shape
        grid = xyz[:, :, [0, 2]].unsqueeze(1)
        s = nn.functional.grid_sample(input=local_latents, grid=grid, mode="bilinear", align_corners=False, padding_mode="zeros")
        return s.permute(0, 2, 3, 1).reshape(B, -1, local_z_dim)

    @staticmethod
    def get_local_coordinates(global_coords, local_grid_length, preserve_y=True):
        """Global [-1, 1] coordinates -> coordinates inside the latent-grid cell, again in [-1, 1] (siren.py:501-518)."""
        local = (global_coords + 1) / 2 * local_grid_length
        local = local - (local - 0.5).round()
        local = local * 2 - 1
        if preserve_y:
            return torch.cat([local[..., 0:1], global_coords[..., 1:2], local[..., 2:3]], dim=-1)
        return local
