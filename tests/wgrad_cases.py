"""Shapes, inputs and fp64 references of the weight-gradient tests (tests/test_gpu_wgrad.py; the parts that need no device are checked by
tests/test_dump_layout_cpu.py).  A plain helper module: numpy, the project's own dump_layout and procedural modules.

The weight-gradient kernels (csrc/fenerf_siren_wgrad.hip) contract the backward dumps over the point axis.  Their inputs already carry
the route's rounding (bf16 in the dump, 2^-17 rev in the 16-bit tape); GIVEN those inputs the result is a plain sum with a definite value.
Everything here is stated on the decoded operands: what is asserted is the contraction, the chunking and the layout, not the route's
precision class."""
import collections
import functools

import numpy as np

from fenerf_amd import dump_layout as DL, procedural as proc

F = np.float32
EPS24 = 2.0 ** -24
DEVICE_CUS = 256           # MI355X; the GPU test repeats the coverage assertion with the device's own count
SMALL_BUDGET = 8           # native.cu_budget(8): few long ragged chunks instead of many one-tile ones


# ---------------------------------------------------------------------------------------------------
# chunk planners, restated from csrc/fenerf_siren_wgrad.hip: wgrad_nchunk, wgrad_nchunk_thin, film_nchunk as functions of (L, B, tiles, CUs)
# ---------------------------------------------------------------------------------------------------
def wgrad_nchunk(L, B, tiles, cus):
    jobs = (L - 1) * B
    best, best_eff = 1, 0.0
    for n in range(1, min(64, tiles) + 1):
        rounds = (jobs * n + cus - 1) // cus
        t_per = (tiles + n - 1) // n
        eff = tiles / (rounds * (t_per + 4)) / cus * jobs
        if eff > best_eff:
            best_eff, best = eff, n
    return best


def wgrad_nchunk_thin(L, B, tiles, cus):
    return max(1, min((2 * cus + B - 1) // B, tiles, 256))


def film_nchunk(tiles):
    return min(tiles, 64)


def workspace_bytes(L, H, B, tiles, cus):
    """wgrad_workspace_bytes restated: the library's scratch size is a function of the three chunk counts, which makes the planners above
    checkable against the library's own (fenerf_siren_grad_workspace_bytes) on the device"""
    nc, nt = wgrad_nchunk(L, B, tiles, cus), wgrad_nchunk_thin(L, B, tiles, cus)
    ncm = max(film_nchunk(tiles), nt)
    f = max((L - 1) * B * nc * H * H, B * nt * H * 160)
    f += L * B * ncm * H * 2 + 2 * B * ncm * 32 + L * B * max(nc, nt) * H
    return (4 * f + 1024 + 255) // 256 * 256              # fenerf_siren_grad_workspace_bytes rounds up to 256 bytes


def chunk_lengths(tiles, nchunk):
    """tiles of every chunk: t_per = ceil(tiles / nchunk), chunk k = [k t_per, min(tiles, (k + 1) t_per)) -- empty past the end"""
    t_per = (tiles + nchunk - 1) // nchunk
    return [max(0, min(tiles, (k + 1) * t_per) - k * t_per) for k in range(nchunk)]


# ---------------------------------------------------------------------------------------------------
# case table
# ---------------------------------------------------------------------------------------------------
class Case(collections.namedtuple("Case", "kind H T B cus")):
    @property
    def P(self):
        return 32 * self.T

    @property
    def id(self):
        return f"{self.kind}-H{self.H}-T{self.T}-B{self.B}-{'cu%d' % self.cus if self.cus else 'dev'}"

    @property
    def seed(self):
        return 1000 * self.H + 10 * self.T + self.B


def _kind(H, T):
    return "baseline" if (T in (2, 7) or H in (96, 192)) else "texture"


CASES = [Case(_kind(H, T), H, T, B, cus) for H in (32, 256) for T in (1, 2, 3, 4, 5, 7, 33) for B in (1, 2) for cus in (0, SMALL_BUDGET)]
CASES += [Case(_kind(H, 5), H, 5, 2, cus) for H in (64, 96, 128, 192) for cus in (0, SMALL_BUDGET)]
CASES += [Case("texture", 32, 300, 1, cus) for cus in (0, SMALL_BUDGET)]       # thin jobs: 256 chunks of 2, 106 empty; FiLM gather: 64 of 5, 4 empty


def spec_of(case):
    return proc.model_spec(case.kind, hidden_dim=case.H, grid_size=6, z_dim=8)


def plans(case, device_cus):
    """-> chunk lengths of the square jobs, the thin jobs and the FiLM gather for this case on a device of `device_cus` CUs"""
    sp = spec_of(case)
    L = sp["n_geo"] + sp["n_color"]
    cus = min(case.cus, device_cus) if case.cus else device_cus
    return (chunk_lengths(case.T, wgrad_nchunk(L, case.B, case.T, cus)), chunk_lengths(case.T, wgrad_nchunk_thin(L, case.B, case.T, cus)),
            chunk_lengths(case.T, film_nchunk(case.T)))


def coverage(device_cus):
    cov = dict(square_lengths=set(), ragged_last=False, thin_empty=False, film_empty=False)
    for c in CASES:
        sq, thin, film = plans(c, device_cus)
        cov["square_lengths"].update(sq)
        cov["ragged_last"] |= len(sq) > 1 and 0 < sq[-1] < sq[0]
        cov["thin_empty"] |= 0 in thin
        cov["film_empty"] |= 0 in film
    return cov


def assert_coverage(cov):
    n = cov["square_lengths"]
    assert {1, 2, 3} <= n, n
    assert any(k >= 4 and k % 2 == 0 for k in n) and any(k >= 4 and k % 2 == 1 for k in n), n
    assert cov["ragged_last"] and cov["thin_empty"] and cov["film_empty"], cov


assert_coverage(coverage(DEVICE_CUS))


# ---------------------------------------------------------------------------------------------------
# routes
# ---------------------------------------------------------------------------------------------------
TAPE_F32, TAPE_U16, TAPE_F32_W = 0, 1, 2           # include/fenerf.h FENERF_TAPE_*
# The default f16x3 / tape16 square job evaluates a product a b of two fp32 operands on the bf16 MFMA as ah bh + ah bl + al bh, fp32
# accumulation.  stage_split4 / stage_split4_pair (fenerf_siren_wgrad.hip) split  hi = the upper 16 bits of the fp32 word -- a TRUNCATION to
# 8 significant bits, so 0 <= |a - ah| < 2^-7 |a| --  and  lo = RNE_bf16(a - ah), so |a - ah - al| <= 2^-9 |a - ah| < 2^-16 |a|.  With
# a = ah + al + ea, b = bh + bl + eb:   a b - (ah bh + ah bl + al bh) = al bl + ea b + a eb - ea eb,  in magnitude below
#     2^-7 2^-7 |a b|  (the dropped lo lo term)  +  2 * 2^-16 |a b|  (the two lo roundings)  =  (2^-14 + 2^-15) |a b| = 3 * 2^-15 |a b|.
# (A split with hi rounded to nearest would halve |al| and give 2^-16 + 2^-16 = 2^-15; this code truncates, which costs the factor 3.
# The products of bf16 pairs themselves are exact in the MFMA's fp32 accumulation step: 16 significant bits.)
C_SPLIT = 3 * 2.0 ** -15
Route = collections.namedtuple("Route", "name precision amp tape_format c_square")
ROUTES = [Route("f32", "f32", 0, TAPE_F32, 0.0), Route("f16x3", "f16x3", 0, TAPE_F32, C_SPLIT), Route("f16x3-w", "f16x3", 0, TAPE_F32_W, C_SPLIT),
          Route("tape16", "f16x3", 0, TAPE_U16, C_SPLIT), Route("amp", "f16x3", 1, TAPE_F32, 0.0), Route("amp-tape16", "f16x3", 1, TAPE_U16, 0.0)]
FACTOR = 4                 # on e32: summation order and device intrinsics, the convention of tests/ray_tail_cases.py value_bound


# ---------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def state_dict(kind, H):
    return proc.make_state_dict(proc.model_spec(kind, hidden_dim=H, grid_size=6, z_dim=8), seed=H + 5, sigma_gain=30.0, with_mapping=False)


@functools.lru_cache(maxsize=None)
def inputs(kind, H, T, B):
    """-> dict(points [B, P, 3] partly outside the +-0.12 box, dirs (unit), film (raw FiLM parameters), d_out (sigma column x 0.02)), float32"""
    case = Case(kind, H, T, B, 0)
    sp = spec_of(case)
    rng = np.random.default_rng(case.seed)
    P = case.P
    pts = rng.uniform(-0.13, 0.13, (B, P, 3)).astype(F)
    dirs = rng.normal(size=(B, P, 3)).astype(F)
    dirs = (dirs / np.linalg.norm(dirs, axis=-1, keepdims=True)).astype(F)
    d_out = rng.normal(size=(B, P, sp["output_dim"])).astype(F)
    d_out[..., -1] *= F(0.02)
    film = proc.film_params(sp, B, seed=case.seed % 97)
    assert (np.abs(pts) > 0.12).any() and (np.abs(pts).max(-1) < 0.12).any()
    for a in (pts, dirs, d_out, *film.values()):
        a.setflags(write=False)
    return dict(points=pts, dirs=dirs, d_out=d_out, film=film)


def film_layers(sd, sp):
    """-> W [L] (nn.Linear layout), b [L] of the FiLM layers, geometry then colour"""
    names = [f"network.{i}.layer" for i in range(sp["n_geo"])] + [f"color_layer_sine.{i}.layer" for i in range(sp["n_color"])]
    return [np.asarray(sd[n + ".weight"], F) for n in names], [np.asarray(sd[n + ".bias"], F) for n in names]


def film_prepared(sd, sp, film, f16x3):
    """What the weight-gradient kernels are handed as (fp, pp) and `inv`, restated from film_prep_prologue (csrc/fenerf_film.h) and the
    packer's result scales (pack_weights_f16, row_scales: csrc/fenerf_pack.cpp):
        f = fl32(fl32(15 f_raw) + 30),   f' = fl32(f / 2 pi * inv),   p' = fl32((f b + p_raw) / 2 pi)    (the divisions in fp64)
        inv[l][n] = 1 / (2^-ex * 16) with max|W_l[n, :]| = m 2^ex, m in [0.5, 1), for the f16x3 layers 1 .. L-1; 1 for layer 0 and at f32
    so that tape * inv = W x.  -> fp, pp [B, L, H] float32, inv [L, H] float32, freq [B, L, H] float64 (= 15 f_raw + 30 in fp64)"""
    H, ng, nc = sp["hidden_dim"], sp["n_geo"], sp["n_color"]
    B = film["freq_geo"].shape[0]
    raw_f = np.concatenate([film["freq_geo"].reshape(B, ng, H), film["freq_app"].reshape(B, nc, H)], 1).astype(F)
    raw_p = np.concatenate([film["phase_geo"].reshape(B, ng, H), film["phase_app"].reshape(B, nc, H)], 1).astype(F)
    W, b = film_layers(sd, sp)
    bias = np.stack(b)
    inv = np.ones((ng + nc, H), F)
    if f16x3:
        for l in range(1, ng + nc):
            m = np.abs(W[l].astype(np.float64)).max(1)
            ex = np.frexp(m)[1]
            inv[l] = np.where(m > 0, np.ldexp(1.0, ex) / 16.0, 1.0 / 16.0).astype(F)
    f = (raw_f * F(15) + F(30)).astype(F)
    inv2pi = 0.15915494309189533576888
    fp = (f.astype(np.float64) * inv2pi * inv.astype(np.float64)).astype(F)
    pp = ((f.astype(np.float64) * bias.astype(np.float64) + raw_p.astype(np.float64)) * inv2pi).astype(F)
    return fp, pp, inv, 15.0 * raw_f.astype(np.float64) + 30.0


# ---------------------------------------------------------------------------------------------------
# contraction: fp64 reference, its fp32 restatement, the magnitude sum, the tile terms
# ---------------------------------------------------------------------------------------------------
def _tiles(a):
    """[B, R, P] -> [B, T, R, 32]"""
    B, R, P = a.shape
    return a.reshape(B, R, P // 32, 32).transpose(0, 2, 1, 3)


def square_tile_terms(A, X, scale):
    """scale[b, n] * sum_{p in tile} A[b, n, p] X[b, k, p]  ->  [B, T, n, k] float64"""
    A, X = np.asarray(A, np.float64), np.asarray(X, np.float64)
    return np.asarray(scale, np.float64)[:, None, :, None] * np.matmul(_tiles(A), _tiles(X).transpose(0, 1, 3, 2))


def square_magnitude(A, X, scale):
    """sum_{b, p} |scale A X| -> [n, k] float64"""
    A, X = np.abs(np.asarray(A, np.float64)), np.abs(np.asarray(X, np.float64))
    return (np.abs(np.asarray(scale, np.float64))[:, :, None] * np.matmul(A, X.transpose(0, 2, 1))).sum(0)


def bound(e32, c, mag, ref, factor=FACTOR):
    """|got - ref64| <= factor * e32 + c * sum |freq dtheta x| + 8 * 2^-24 * max|ref64|, per element"""
    ref = np.asarray(ref)
    return factor * e32 + c * np.asarray(mag) + 8 * EPS24 * (float(np.abs(ref).max()) if ref.size else 0.0)


def insensitive_tiles(terms, bnd):
    """(image, tile) pairs whose removal moves NO element of the sum by more than twice the bound"""
    hit = (np.abs(terms) > 2 * bnd).any((2, 3))
    return [(int(b), int(t)) for b, t in zip(*np.nonzero(~hit))]


Check = collections.namedtuple("Check", "ref e32 mag c insensitive")


def _ones(B, R):
    return np.ones((B, R))


def contract(A64, X64, A32, X32, scale64, scale32, c=0.0, sensitivity=False):
    """ref64 = sum_b diag(scale_b) sum_p A X^T and the same statement in float32 (products, sums per 32-point tile, then over the tiles,
    then the scale and the images) -> Check, and the per-image unscaled sums G64, G32 [B, n, k]"""
    t64 = np.matmul(_tiles(A64), _tiles(X64).transpose(0, 1, 3, 2))                  # [B, T, n, k]
    G64 = t64.sum(1)
    ref = (scale64[:, :, None] * G64).sum(0)
    t32 = np.matmul(_tiles(A32), _tiles(X32).transpose(0, 1, 3, 2))
    assert t32.dtype == F
    G32 = np.zeros(G64.shape, F)
    for t in range(t32.shape[1]):
        G32 += t32[:, t]
    r32 = np.zeros(ref.shape, F)
    for b in range(G32.shape[0]):
        r32 += scale32[b][:, None] * G32[b]
    e32 = float(np.abs(r32.astype(np.float64) - ref).max())
    mag = square_magnitude(A64, X64, scale64)
    ins = None
    if sensitivity:
        ins = insensitive_tiles(scale64[:, None, :, None] * t64, bound(e32, c, mag, ref))
    return Check(ref, e32, mag, c, ins), G64, G32


def _sin64(rev):
    return np.sin(2.0 * np.pi * rev)


def _sin32(rev32):
    return np.sin(F(2.0 * np.pi) * rev32, dtype=F)


def reference(route, sp, sd, inp, bufs, d_phase_got=None):
    """fp64 references of every tensor fenerf_siren_param_grads returns that is a function of decodable operands on this route.
    bufs: numpy copies of what the kernels were handed -- tape, d_t (flat float32), out, d_out [B, P, C], tape_e [B P, 32] or None.
    d_phase_got [B, L, H]: the call's own phase gradients, an OPERAND of the frequency gradients that are derived from the weight sums on a
    bf16-dump route (there the chain kernel's FiLM sums are taken before the bf16 rounding and cannot be decoded from the dump).
    -> {name: Check}; names as in NativeModel.siren_param_grads, list entries as 'geo_w.3'."""
    H, ng, nc, G, C = sp["hidden_dim"], sp["n_geo"], sp["n_color"], sp["grid_ch"], sp["output_dim"]
    L, n_lab = ng + nc, sp["output_dim"] - 4
    B, P, _ = inp["points"].shape
    T = P // 32
    f16x3 = route.precision == "f16x3"
    fp, pp, inv, freq64 = film_prepared(sd, sp, inp["film"], f16x3)
    freq32 = (np.concatenate([inp["film"]["freq_geo"].reshape(B, ng, H), inp["film"]["freq_app"].reshape(B, nc, H)], 1) * F(15) + F(30)).astype(F)
    W, bias = film_layers(sd, sp)
    u16 = route.tape_format == TAPE_U16
    from_sums = route.tape_format != TAPE_F32

    # ---- operands, as the route's kernels obtain them
    if route.amp:
        dth, x_dump = DL.decode_bf16_dump(bufs["d_t"], L, H, B, T)
    else:
        dth, x_dump = DL.decode_f32_dump(bufs["d_t"], L, H, B, T), None
    if u16:
        phase = DL.tape16_phase(DL.decode_tape16(bufs["tape"], L, H, B, T))
        tape = None
    else:
        tape = DL.decode_f32_dump(bufs["tape"], L, H, B, T)

    memo = {}

    def x_from_tape(l):
        if l not in memo:
            memo[l] = _x_from_tape(l)
        return memo[l]

    def _x_from_tape(l):
        if u16:
            return _sin64(phase[l].astype(np.float64)), _sin32(phase[l])
        a64 = fp[:, l, :, None].astype(np.float64) * tape[l].astype(np.float64) + pp[:, l, :, None].astype(np.float64)
        a32 = fp[:, l, :, None] * tape[l] + pp[:, l, :, None]
        return _sin64(a64), _sin32(a32)

    def x_square(l):
        if route.amp:
            return x_dump[l].astype(np.float64), x_dump[l]
        return x_from_tape(l)

    box = F(2 / 0.24)
    warped64 = (inp["points"].astype(np.float64) * float(box)).transpose(0, 2, 1)              # [B, 3, P]
    warped32 = (inp["points"] * box).transpose(0, 2, 1)
    dirs32 = np.ascontiguousarray(inp["dirs"].transpose(0, 2, 1))
    side32 = dirs32 if not G else np.concatenate([dirs32, bufs["tape_e"].reshape(B, P, 32).transpose(0, 2, 1)], 1)   # [B, 3 + G, P]

    res = {}
    G_of = {}                                                        # per-image unscaled sums per layer: (G64, G32, columns that carry c)
    for l in range(L):
        a32 = dth[l]
        a64 = a32.astype(np.float64)
        s64, s32 = freq64[:, l], freq32[:, l]
        name = f"geo_w.{l}" if l < ng else f"color_w.{l - ng}"
        if l == 0:
            chk, g64, g32 = contract(a64, warped64, a32, warped32, s64, s32)
            res[name] = chk
            G_of[l] = (g64, g32, np.zeros(3, bool))
            continue
        x64, x32 = x_square(l - 1)
        chk, g64, g32 = contract(a64, x64, a32, x32, s64, s32, c=route.c_square, sensitivity=True)
        if l != ng:
            res[name] = chk
            G_of[l] = (g64, g32, np.ones(H, bool))
            continue
        thin, t64, t32 = contract(a64, side32.astype(np.float64), a32, side32, s64, s32)
        res[name + ".x"] = chk                                       # columns 3 + G .. of colour layer 0: the square job
        res[name + ".side"] = thin                                   # columns 0 .. 3 + G: view direction, grid features (thin job C0X)
        G_of[l] = (np.concatenate([t64, g64], 2), np.concatenate([t32, g32], 2), np.arange(3 + G + H) >= 3 + G)

    # ---- heads: the left operand as the WG_HEAD / WG_RGB staging forms it
    d_out, out = bufs["d_out"].reshape(B, P, C), bufs["out"].reshape(B, P, C)
    head_a = np.zeros((B, 32, P), F)
    head_a[:, :n_lab] = d_out[:, :, :n_lab].transpose(0, 2, 1)       # row r < n_lab: label channel r
    head_a[:, n_lab] = d_out[:, :, C - 1]                            # row n_lab: sigma
    x64, x32 = x_from_tape(ng - 1)
    chk, _, _ = contract(head_a.astype(np.float64), x64, head_a, x32, _ones(B, 32), np.ones((B, 32), F))
    res["head_w"] = chk
    res["head_b"] = _rowsum(head_a)
    rgb, d_rgb = out[:, :, C - 4:C - 1].transpose(0, 2, 1), d_out[:, :, C - 4:C - 1].transpose(0, 2, 1)
    rgb_a64 = d_rgb.astype(np.float64) * (rgb.astype(np.float64) * (1.0 - rgb.astype(np.float64)))
    rgb_a32 = (d_rgb * (rgb * (F(1) - rgb))).astype(F)
    x64, x32 = x_from_tape(L - 1)
    chk, _, _ = contract(rgb_a64, x64, rgb_a32, x32, _ones(B, 3), np.ones((B, 3), F))
    res["rgb_w"] = chk
    res["rgb_b"] = _rowsum(rgb_a32, rgb_a64)

    # ---- FiLM sums
    d_phase = d_freq = None
    if not route.amp:                                               # fp32 dump: the chain kernel's per-tile sums against its own dump
        s0 = [_rowsum(dth[l], per_image=True) for l in range(L)]
        d_phase = _stack_checks(s0)
        for l in range(L):
            # d_bias_l = sum_b freq_bl d_phase_bl
            r = (freq64[:, l] * s0[l].ref).sum(0)
            r32 = np.zeros(H, F)
            for b in range(B):
                r32 += freq32[b, l] * s0[l].ref32[b]
            e = float(np.abs(r32 - r).max())
            res[(f"geo_b.{l}" if l < ng else f"color_b.{l - ng}")] = Check(r, e, (freq64[:, l] * s0[l].mag).sum(0), 0.0, None)
    if not from_sums and not route.amp:                             # d_freq = 15 sum_p dtheta (tape inv + b): the chain kernel's second sum
        fr = []
        for l in range(L):
            a64, t64 = dth[l].astype(np.float64), tape[l].astype(np.float64)
            iv, bb = inv[l].astype(np.float64)[None, :], bias[l].astype(np.float64)[None, :]
            s1 = (a64 * t64).sum(-1)
            r = 15.0 * (s1 * iv + s0[l].ref * bb)
            s1_32 = _tile_sum32(dth[l] * tape[l])
            r32 = F(15) * (s1_32 * inv[l][None, :] + s0[l].ref32 * bias[l][None, :])
            mag = 15.0 * (np.abs(a64 * t64).sum(-1) * iv + s0[l].mag * np.abs(bb))
            fr.append(_Sum(r, r32.astype(F), float(np.abs(r32 - r).max()), mag))
        d_freq = _stack_checks(fr)
    if from_sums:                                                   # d_freq = 15 (b d_phase + sum_k W[n, k] G_b[n, k]), the weight sums' own G
        fr = []
        for l in range(L):
            g64, g32, cc = G_of[l]
            w64 = W[l].astype(np.float64)
            if route.amp:
                dp64, dp32, dpm = d_phase_got[:, l].astype(np.float64), d_phase_got[:, l].astype(F), np.abs(d_phase_got[:, l].astype(np.float64))
            else:
                dp64, dp32, dpm = s0[l].ref, s0[l].ref32, s0[l].mag
            bb = bias[l].astype(np.float64)[None, :]
            r = 15.0 * (bb * dp64 + (w64[None] * g64).sum(-1))
            r32 = F(15) * (bias[l][None, :] * dp32 + (W[l][None] * g32).sum(-1, dtype=F))
            # magnitude of the products that go through the split: |W| sum_p |dtheta x| over the square job's columns
            absG = np.matmul(np.abs(dth[l].astype(np.float64)), np.abs(_layer_input64(l, x_square, warped64, side32, ng)).transpose(0, 2, 1))
            mag_c = 15.0 * (np.abs(w64)[None] * absG * cc[None, None, :]).sum(-1)
            mag = 15.0 * ((np.abs(w64)[None] * absG).sum(-1) + np.abs(bb) * dpm)
            fr.append(_Sum(r, r32.astype(F), float(np.abs(r32 - r).max()), mag, route.c_square * mag_c))
        d_freq = _stack_checks(fr)
    for key, stack in (("d_phase", d_phase), ("d_freq", d_freq)):
        if stack is not None:
            res[key + "_geo"] = _slice_check(stack, 0, ng)
            res[key + "_app"] = _slice_check(stack, ng, L)
    return res


def _layer_input64(l, x_square, warped64, side32, ng):
    if l == 0:
        return warped64
    x = x_square(l - 1)[0]
    return x if l != ng else np.concatenate([side32.astype(np.float64), x], 1)


class _Sum:
    """a per-image row quantity [B, H]: fp64 value, its fp32 restatement, e32, magnitude, an extra absolute allowance"""
    def __init__(self, ref, ref32, e32, mag, extra=0.0):
        self.ref, self.ref32, self.e32, self.mag, self.extra = ref, ref32, e32, mag, extra


def _tile_sum32(v32):
    """[B, H, P] float32 -> [B, H]: sums per 32-point tile, then over the tiles, in float32"""
    B, R, P = v32.shape
    t = v32.reshape(B, R, P // 32, 32).sum(-1, dtype=F)
    s = np.zeros((B, R), F)
    for k in range(t.shape[2]):
        s += t[:, :, k]
    return s


def _rowsum(a32, a64=None, per_image=False):
    a64 = a32.astype(np.float64) if a64 is None else a64
    r, r32, mag = a64.sum(-1), _tile_sum32(a32), np.abs(a64).sum(-1)
    if per_image:
        return _Sum(r, r32, float(np.abs(r32 - r).max()), mag)
    r, mag = r.sum(0), mag.sum(0)
    s = np.zeros(r.shape, F)
    for b in range(r32.shape[0]):
        s += r32[b]
    return Check(r, float(np.abs(s - r).max()), mag, 0.0, None)


class _Stack:
    def __init__(self, ref, e32, extra):
        self.ref, self.e32, self.extra = ref, e32, extra


def _stack_checks(sums):
    """[L] per-image row quantities -> [B, L, H] with one e32 (the max over the layers: they are one returned tensor)"""
    ref = np.stack([s.ref for s in sums], 1)
    extra = np.stack([np.broadcast_to(s.extra, s.ref.shape) for s in sums], 1)
    return _Stack(ref, [s.e32 for s in sums], extra)


def _slice_check(stack, l0, l1):
    B = stack.ref.shape[0]
    ref = stack.ref[:, l0:l1].reshape(B, -1)
    # `mag` carries the ready-made c * magnitude term (c = 1): the split only enters the frequency gradients derived from the weight sums
    return Check(ref, max(stack.e32[l0:l1]), stack.extra[:, l0:l1].reshape(B, -1), 1.0, None)


# ---------------------------------------------------------------------------------------------------
# synthetic bf16 dump with exact operands
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def synthetic_dump(L, H, B, T, seed):
    """d theta: integers in [-4, 4]; x: multiples of 2^-7 in [-1, 1] -- both exact in bf16, every product a multiple of 2^-7 below 4 and every
    partial sum of up to 9,600 of them below 2^24 * 2^-7: exact in fp32 in any order.  -> (d theta, x) float32 [L, B, H, 32 T], the dump"""
    rng = np.random.default_rng(seed)
    dth = rng.integers(-4, 5, size=(L, B, H, 32 * T)).astype(F)
    x = (rng.integers(-128, 129, size=(L, B, H, 32 * T)) / 128.0).astype(F)
    assert 32 * T * 4 * 128 < 2 ** 24
    dump = DL.encode_bf16_dump(dth, x)
    for a in (dth, x, dump):
        a.setflags(write=False)
    return dth, x, dump
