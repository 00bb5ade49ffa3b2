"""The per-point-modulated family (SPATIALSIRENGRID) against fp64, at every instantiated hidden width and at the edges of its launch
arithmetic: fenerf_siren_forward_local (mapping network + SIREN in one launch) and fenerf_siren_forward_pointwise (explicit [B, P, 9H]
FiLM tensors), the widths between the instantiated ones (zero padding), the slab walk of the explicit route and ray_dirs = None.

Every reference is oracle/ in fp64 (O.mapping_network, O.siren_forward) on the same fp32 inputs the kernels get; the fp32 numpy oracle's
own error against fp64 is printed beside each figure, so that a reader sees the fp32 class."""
import numpy as np
import pytest
import torch

from fenerf_amd import _lib, native
from fenerf_amd.siren import siren as S
from oracle import fenerf_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


def N_(t):
    return t.detach().cpu().numpy()


WIDTHS = [32, 64, 96, 128, 192, 256]          # native.SUPPORTED_HIDDEN
# (B, P) from the launch arithmetic of fenerf_siren_local.hip / the pointwise forward: grid = persistent_blocks(tiles, 4, cus), nx =
# min(blocks, 8) contiguous tile ranges of blocks / nx (+ 1) workgroups of 4 waves, one 32-point tile per wave and loop iteration
SHAPES = [(1, 1),          # one partial tile, three idle waves, 31 lanes clamped to pt = P - 1
          (1, 31),         # the same with one clamped lane
          (1, 33),         # a full tile and a 1-point tile
          (3, 37),         # 111 points: the images straddle tile boundaries (the local kernel sees B * P merged)
          (1, 160),        # 5 tiles: 2 workgroups, nx = 2, uneven ranges [0, 2) and [2, 5)
          (1, 1179)]       # 37 tiles: 10 workgroups, nx = 8, blocks % 8 != 0; ranges of 5 tiles on one workgroup (wave 0 loops twice); ragged end

# max|err| against fp64 inside the init range, (rgb, sigma relative to max(1, max|sigma|)), per route and width: the largest value measured
# on an MI355X over every case that runs at that width -- SHAPES, the at-scale cases (32, 96), the padded widths below (24 -> 32, 72 -> 96,
# 100 -> 128, 200 -> 256) and the injection-free calls of tests/test_gpu_nonfinite.py (32, 72 -> 96).  Asserted: 1.5 x these (_bound).  The
# fp32 numpy oracle is in the same class on the same inputs (rgb 0.8e-6 .. 4.2e-6, sigma 1.5e-5 .. 3.7e-5: the [parity] lines).
MEASURED = {
    # H: ((one-launch local kernel rgb, sigma), (explicit per-point kernel rgb, sigma))
    32: ((4.50e-6, 5.16e-5), (3.29e-6, 3.50e-5)),          # the worst of each at 65,927 points (at scale); <= 1.62e-6 / 3.71e-5 below 1,200 points
    64: ((1.35e-6, 3.03e-5), (9.17e-7, 2.79e-5)),
    96: ((1.96e-6, 3.71e-5), (1.28e-6, 3.15e-5)),
    128: ((1.04e-6, 2.43e-5), (9.29e-7, 2.15e-5)),
    192: ((1.10e-6, 2.77e-5), (8.24e-7, 2.06e-5)),
    256: ((1.35e-6, 3.05e-5), (9.86e-7, 2.57e-5)),
}
FINDING = 1e-4          # what test_spatial_siren_grid_vs_reference asserts for the explicit route: an error above it is a bug, not a tolerance


def _bound(Hp):
    f, x = MEASURED[Hp]
    assert max(f + x) <= FINDING
    return (1.5 * f[0], 1.5 * f[1]), (1.5 * x[0], 1.5 * x[1])


def _module(H, seed=3):
    """SPATIALSIRENGRID in eval mode, init-range weights; final_layer.weight x 20 so that sigma is not tiny (as
    test_gpu_parity.py::test_pointwise_siren_backward_native_vs_fp64_autograd)"""
    torch.manual_seed(seed)
    mod = S.SPATIALSIRENGRID(input_dim=3, z_dim=16, hidden_dim=H, output_dim=4).to(DEV).eval()
    mod.device = torch.device(DEV)
    with torch.no_grad():
        mod.final_layer.weight.mul_(20.0)
    return mod


def _inputs(B, P, seed=4):
    """random points in the +-0.12 box, unit directions, a random [B, 32, 32, 32] latent grid"""
    g_ = torch.Generator(device=DEV).manual_seed(seed)
    pts = (torch.rand((B, P, 3), device=DEV, generator=g_) - 0.5) * 0.24
    dirs = torch.nn.functional.normalize(torch.randn((B, P, 3), device=DEV, generator=g_), dim=-1)
    lat = torch.randn((B, 32, 32, 32), device=DEV, generator=g_)
    return pts, dirs, lat


def _both_routes(mod, pts, dirs, lat):
    """-> dict(fused, explicit, sampled, local, f, p): the one-launch route, and the explicit route on the fp32 FiLM tensors torch's mapping
    network produced"""
    with torch.no_grad():
        fused = mod.forward_with_latent_grid(pts, lat, dirs)
        sampled = mod.sample_local_latents(lat, mod.gridwarper(pts))
        f, p = mod.mapping_network(sampled)
        local = mod.get_local_coordinates(pts, 32, preserve_y=False)
        explicit = mod.forward_with_frequencies_phase_shifts(local, f, p, dirs)
    return dict(fused=fused, explicit=explicit, sampled=sampled, local=local, f=f, p=p)


def _errors(mod, r, dirs, chunk=4096):
    """max|err| against fp64 of both routes, (rgb, sigma relative), and of the fp32 numpy oracle: the fp64 mapping network and SIREN on the
    same fp32 sampled latents and local coordinates (fused route); the fp64 SIREN on exactly the fp32 FiLM tensors (explicit route).  Walked
    in chunks of a few thousand points: the [n, 9H] FiLM blocks in fp64 stay small."""
    sd, spec = mod._state_numpy(), mod._spec()
    msd = {"m.network." + n: N_(q).astype(np.float64) for n, q in mod.mapping_network.network.named_parameters()}
    flat = lambda t: t.reshape(1, -1, t.shape[-1])
    fused, explicit, sampled, local, f, p = (flat(r[k]) for k in ("fused", "explicit", "sampled", "local", "f", "p"))
    dirs = flat(dirs)
    n = fused.shape[1]
    e = np.zeros((3, 2))          # rows: fused, explicit, fp32 oracle; columns: rgb, sigma (absolute here)
    smax = 0.0
    for s in range(0, n, chunk):
        c = slice(s, s + chunk)
        lo, di = N_(local[:, c]), N_(dirs[:, c])
        f64, p64 = O.mapping_network(msd, "m", N_(sampled[:, c]).astype(np.float64))
        o_fused = O.siren_forward(sd, spec, lo, di, f64, p64, dtype=np.float64)
        fc, pc = N_(f[:, c]), N_(p[:, c])
        o_expl = O.siren_forward(sd, spec, lo, di, fc, pc, dtype=np.float64)
        o32 = O.siren_forward(sd, spec, lo, di, fc, pc, dtype=np.float32)
        for row, (got, ref) in enumerate(((N_(fused[:, c]), o_fused), (N_(explicit[:, c]), o_expl), (o32, o_expl))):
            d = np.abs(got - ref)
            assert np.isfinite(got).all()
            e[row] = np.maximum(e[row], (d[..., :3].max(), d[..., 3].max()))
        smax = max(smax, float(np.abs(o_expl[..., 3]).max()))
    e[:, 1] /= max(1.0, smax)
    return e, smax


def _check(tag, H, e, smax):
    Hp = native.padded_hidden_dim(H)
    (bf_rgb, bf_sig), (bx_rgb, bx_sig) = _bound(Hp)
    print(f"[parity] per-point FiLM inside the init range {tag}: max|err| vs fp64 -- one-launch local kernel rgb {e[0, 0]:.2e} sigma rel {e[0, 1]:.2e}; "
          f"explicit per-point kernel rgb {e[1, 0]:.2e} sigma rel {e[1, 1]:.2e}; fp32 numpy oracle rgb {e[2, 0]:.2e} sigma rel {e[2, 1]:.2e} "
          f"(|sigma| max {smax:.2f}); bounds at width {Hp}: {bf_rgb:.2e} {bf_sig:.2e} / {bx_rgb:.2e} {bx_sig:.2e}")
    # 1.5 x the per-width maxima measured on an MI355X (MEASURED above: e.g. width 256 one-launch rgb 1.35e-6 / sigma 3.05e-5, explicit 9.86e-7 / 2.57e-5)
    assert e[0, 0] <= bf_rgb and e[0, 1] <= bf_sig, (tag, "one-launch local kernel", e[0].tolist())
    assert e[1, 0] <= bx_rgb and e[1, 1] <= bx_sig, (tag, "explicit per-point kernel", e[1].tolist())


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. forward against fp64 at every instantiated width
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,P", SHAPES)
@pytest.mark.parametrize("H", WIDTHS)
def test_pointwise_and_local_forward_vs_fp64_at_every_width(H, B, P):
    """The two native routes share mfma_x, the weight ring and the packer's ring padding (KGXP = pad_pf(KGX), KGCP differ per width): compared
    with each other a shared mistake cancels, so each is held to fp64 on its own."""
    mod = _module(H)
    pts, dirs, lat = _inputs(B, P, seed=H + P)
    r = _both_routes(mod, pts, dirs, lat)
    assert r["fused"].shape == r["explicit"].shape == (B, P, 4)
    e, smax = _errors(mod, r, dirs)
    _check(f"H={H} B={B} P={P}", H, e, smax)


@pytest.mark.parametrize("H", [32, 96])
def test_pointwise_and_local_forward_vs_fp64_at_scale(H):
    """32 (8 cus + 12) + 7 points: every wave of the persistent grid runs its tile loop two or three times at whatever CU count the device
    reports (weight ring re-primed, LDS stage reused), and the last tile is ragged."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    total = 32 * (8 * cus + 12) + 7
    mod = _module(H)
    pts, dirs, lat = _inputs(1, total, seed=H)
    r = _both_routes(mod, pts, dirs, lat)
    e, smax = _errors(mod, r, dirs)
    _check(f"H={H} at scale, {total} points on {cus} CUs", H, e, smax)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. widths between the instantiated ones on the no-grad routes: the padded network, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------------------
def _pad_blocks(t, n, H, Hp):
    """[..., n * H] -> [..., n * Hp], zeros behind every block"""
    return torch.nn.functional.pad(t.reshape(*t.shape[:-1], n, H), (0, Hp - H)).reshape(*t.shape[:-1], n * Hp)


def _padded_twin(mod, H, Hp):
    """the same network built at width Hp: every parameter zero-padded (the mapping network's last layer as [2][L][H] -> [2][L][Hp])"""
    twin = S.SPATIALSIRENGRID(input_dim=3, z_dim=16, hidden_dim=Hp, output_dim=4).to(DEV).eval()
    twin.device = torch.device(DEV)
    L = len(mod.network) + 1
    src = dict(mod.named_parameters())
    with torch.no_grad():
        for n, q in twin.named_parameters():
            t = src[n].detach()
            if n.startswith("grid_latent_network"):
                pass
            elif n == "mapping_network.network.4.weight":
                t = torch.nn.functional.pad(t.reshape(2, L, H, -1), (0, 0, 0, Hp - H)).reshape(2 * L * Hp, -1)
            elif n == "mapping_network.network.4.bias":
                t = _pad_blocks(t, 2 * L, H, Hp)
            elif mod._is_render_param(n):
                t = native._pad_param(n, t, H, Hp, 0, False)
            assert t.shape == q.shape, (n, tuple(t.shape), tuple(q.shape))
            q.copy_(t)
    return twin


@pytest.mark.parametrize("H", [24, 72, 100, 200])
def test_width_between_the_instantiated_ones_on_the_no_grad_routes(H):
    """include/fenerf.h promises any hidden width up to 256 through zero padding: both no-grad routes run, are within the bound of their
    padded width against fp64 of the UNPADDED network, and equal the module built at the padded width with zero-padded parameters bit for bit
    (what test_hidden_width_between_the_instantiated_ones_is_the_padded_network_bit_for_bit states for the per-image path)."""
    B, P = 2, 70
    Hp = native.padded_hidden_dim(H)
    L = 9
    mod = _module(H)
    pts, dirs, lat = _inputs(B, P, seed=H)
    r = _both_routes(mod, pts, dirs, lat)
    assert mod.native_local(DEV).spec["hidden_dim"] == Hp == mod.native(DEV).spec["hidden_dim"] and mod.native(DEV).logical_H == H
    e, smax = _errors(mod, r, dirs)
    _check(f"H={H} (run at {Hp}) B={B} P={P}", H, e, smax)
    twin = _padded_twin(mod, H, Hp)
    with torch.no_grad():
        fused_p = twin.forward_with_latent_grid(pts, lat, dirs)
        explicit_p = twin.forward_with_frequencies_phase_shifts(r["local"], _pad_blocks(r["f"], L, H, Hp), _pad_blocks(r["p"], L, H, Hp), dirs)
    assert torch.equal(r["fused"], fused_p), "one-launch local kernel: not the padded network"
    assert torch.equal(r["explicit"], explicit_p), "explicit per-point kernel: not the padded network"
    # FiLM tensors of a wrong width are refused in terms of the module's own width
    fg, pg, fa, pa = mod.split_film(r["f"], r["p"])
    with pytest.raises(ValueError, match=rf"expected \({B}, {P}, {8 * H}\)"):
        mod.native(DEV).siren_forward_pointwise(r["local"], dirs, fg[..., :-1], pg, fa, pa)


def test_width_beyond_the_largest_instantiated_one_names_the_limit():
    mod = _module(300)
    pts, dirs, lat = _inputs(1, 33)
    with torch.no_grad():
        with pytest.raises(ValueError, match="hidden_dim 300: the kernels are instantiated up to 256"):
            mod.forward_with_latent_grid(pts, lat, dirs)
        sampled = mod.sample_local_latents(lat, mod.gridwarper(pts))
        f, p = mod.mapping_network(sampled)
        with pytest.raises(ValueError, match="hidden_dim 300: the kernels are instantiated up to 256"):
            mod.forward_with_frequencies_phase_shifts(pts, f, p, dirs)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. the slab walk of the explicit route
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_pointwise_forward_slab_walk_equals_one_slab(monkeypatch):
    """siren_forward_pointwise walks the points of an image in slabs so that its FiLM scratch stays near native.POINTWISE_FILM_SCRATCH_BYTES
    (14,560 points at H = 256).  Lowered so that a slab is one 32-point tile, (B, P) = (2, 100) walks 32 + 32 + 32 + 4 points per image;
    rows are independent, so the result is the single-slab call's bit for bit.  The FiLM tensors once as non-contiguous views."""
    H, B, P, L = 32, 2, 100, 9
    mod = _module(H)
    pts, dirs, lat = _inputs(B, P, seed=9)
    r = _both_routes(mod, pts, dirs, lat)          # unpatched: one slab per image
    nat = mod.native(DEV)
    l = _lib.lib()
    walked = []
    real = l.fenerf_film_workspace_bytes_pointwise

    def spy(h, b, n):
        walked.append((int(b), int(n)))
        return real(h, b, n)
    monkeypatch.setattr(l, "fenerf_film_workspace_bytes_pointwise", spy)
    with torch.no_grad():
        mod.forward_with_frequencies_phase_shifts(r["local"], r["f"], r["p"], dirs)
    assert walked == [(1, P)] * B, walked
    assert native.POINTWISE_FILM_SCRATCH_BYTES == 1 << 28
    monkeypatch.setattr(native, "POINTWISE_FILM_SCRATCH_BYTES", 32 * 8 * L * H)
    del walked[:]
    with torch.no_grad():
        slabbed = mod.forward_with_frequencies_phase_shifts(r["local"], r["f"], r["p"], dirs)
    assert walked == [(1, 32), (1, 32), (1, 32), (1, 4)] * B, walked
    assert torch.equal(slabbed, r["explicit"])
    # non-contiguous FiLM views (slices of a wider tensor) straight into the native call
    wide_f = torch.cat([torch.full_like(r["f"][..., :5], 7.0), r["f"], torch.full_like(r["f"][..., :3], -7.0)], -1)
    wide_p = torch.cat([torch.full_like(r["p"][..., :5], 7.0), r["p"], torch.full_like(r["p"][..., :3], -7.0)], -1)
    fv, pv = wide_f[..., 5:5 + L * H], wide_p[..., 5:5 + L * H]
    views = (fv[..., :8 * H], pv[..., :8 * H], fv[..., 8 * H:], pv[..., 8 * H:])
    assert not any(v.is_contiguous() for v in views)
    del walked[:]
    got = nat.siren_forward_pointwise(r["local"], dirs, *views)
    assert walked == [(1, 32), (1, 32), (1, 32), (1, 4)] * B and torch.equal(got, r["explicit"])
    print(f"[parity] per-point FiLM slab walk H={H} B={B} P={P}: {len(walked)} slabs of {[n for _, n in walked[:4]]} points per image, contiguous and "
          f"non-contiguous FiLM tensors: bit-identical to the single-slab call")


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. ray_dirs = None: both kernels substitute (0, 0, -1)
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_ray_dirs_none_is_the_direction_0_0_minus_1():
    H, B, P = 64, 2, 70
    mod = _module(H)
    pts, _, lat = _inputs(B, P, seed=11)
    dirs = torch.zeros((B, P, 3), device=DEV)
    dirs[..., 2] = -1.0
    r = _both_routes(mod, pts, dirs, lat)
    with torch.no_grad():
        fused = mod.forward_with_latent_grid(pts, lat, None)
        explicit = mod.forward_with_frequencies_phase_shifts(r["local"], r["f"], r["p"], None)
    other = _both_routes(mod, pts, torch.nn.functional.normalize(torch.ones_like(dirs), dim=-1), lat)
    moved = (other["fused"][..., :3] - r["fused"][..., :3]).abs().max().item()
    print(f"[parity] per-point FiLM ray_dirs=None H={H} B={B} P={P}: both routes bit-identical to explicit (0, 0, -1) directions "
          f"(another direction moves rgb by {moved:.2e})")
    assert torch.equal(fused, r["fused"]) and torch.equal(explicit, r["explicit"])
    assert moved > 1e-5, "the direction must matter for the comparison to say anything"
