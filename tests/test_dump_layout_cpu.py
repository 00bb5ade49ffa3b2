"""fenerf_amd/dump_layout.py against csrc/fenerf_layout.h, on the host: the index functions as the header states them (in words and as
the MFMA C/D layout they come from), every (feature, point) pair of a tile hit exactly once, encode -> decode the identity at every
instantiated width.  The planner coverage of tests/wgrad_cases.py and its tile-sensitivity condition are evaluated here too, on a
synthetic reference, so that a machine without a GPU checks them."""
import numpy as np
import pytest

from fenerf_amd import dump_layout as DL

import wgrad_cases as WC

WIDTHS = [32, 64, 96, 128, 192, 256]


def feat_of(s, h):
    """fenerf_layout.h: accumulator register r = s & 15 of n-block s >> 4, lane half h: row (r & 3) + 8 (r >> 2) + 4 h"""
    return 32 * (s >> 4) + (s & 3) + 8 * ((s & 15) >> 2) + 4 * h


def test_widths_are_the_instantiated_ones():
    assert list(DL.WIDTHS) == WIDTHS


@pytest.mark.parametrize("H", WIDTHS)
def test_index_functions_equal_the_header(H):
    for g in range(H // 8):
        nb, j = g >> 2, g & 3
        for half in range(2):
            for i in range(4):
                # "element i of lane (m, half) in group g = 4 nb + j is feature 32 nb + 8 j + 4 half + i": registers 4 j + i of the n-block
                assert DL.tape_feature(g, half, i) == 32 * nb + 8 * j + 4 * half + i == feat_of(16 * nb + 4 * j + i, half)
    for nb in range(H // 32):
        for g in range(4):
            for rt in range(2):
                for r in range(4):
                    # "lane (n, g) slot t = 4 rt + r: feature 32 nb + 16 (g >> 1) + 4 (g & 1) + 8 rt + r"
                    assert DL.dump16_feature(nb, g, 4 * rt + r) == 32 * nb + 16 * (g >> 1) + 4 * (g & 1) + 8 * rt + r


@pytest.mark.parametrize("H", WIDTHS)
def test_every_feature_point_pair_of_a_tile_exactly_once(H):
    for index in (DL.f32_dump_index, DL.dump16_index):
        feat, pt = index(H)
        assert feat.shape == pt.shape == (H * 32,)
        assert feat.min() == 0 and feat.max() == H - 1 and pt.min() == 0 and pt.max() == 31
        hits = np.zeros((H, 32), np.int64)
        np.add.at(hits, (feat, pt), 1)
        assert (hits == 1).all()


def test_storage_order_of_the_first_values():
    """spot values read off the header by hand, H = 64: float 4 * (64 g + lane) + i of an fp32 block; u16 8 * (128 nb + 64 odd + lane) + t"""
    feat, pt = DL.f32_dump_index(64)
    k = 4 * (64 * 5 + 37) + 2                  # g = 5 (nb 1, j 1), lane 37 (m 5, half 1), i = 2
    assert (feat[k], pt[k]) == (32 + 8 + 4 + 2, 5)
    feat, pt = DL.dump16_index(64)
    k = 8 * (128 * 1 + 64 * 1 + 45) + 6        # nb 1, odd tile, lane 45 (n 13, g 2), slot 6 (rt 1, r 2)
    assert (feat[k], pt[k]) == (32 + 16 + 0 + 8 + 2, 16 + 13)


@pytest.mark.parametrize("H", WIDTHS)
def test_encode_then_decode_is_the_identity(H):
    rng = np.random.default_rng(H)
    L, B, T = 3, 2, 3
    v = rng.normal(size=(L, B, H, 32 * T)).astype(np.float32)
    buf = DL.encode_f32_dump(v)
    assert buf.dtype == np.float32 and buf.size == DL.f32_dump_floats(L, H, B, T)
    assert np.array_equal(DL.decode_f32_dump(np.concatenate([buf, np.ones(7, np.float32)]), L, H, B, T), v)
    # storage order: the value of (tile, layer, g, lane, i) sits where the header says
    b, t, l, g, lane, i = 1, 2, 1, H // 8 - 1, 41, 3
    assert buf.reshape(B, T, L, H // 8, 64, 4)[b, t, l, g, lane, i] == v[l, b, DL.tape_feature(g, lane >> 5, i), 32 * t + (lane & 31)]

    d = DL.bf16_to_f32(DL.bf16_round(v))               # bf16-exact values survive the round trip bit for bit
    x = DL.bf16_to_f32(DL.bf16_round(np.sin(v)))
    dump = DL.encode_bf16_dump(d, x)
    assert dump.dtype == np.float32 and dump.size == DL.f32_dump_floats(L, H, B, T)      # the same H * 128 bytes per block
    d2, x2 = DL.decode_bf16_dump(dump, L, H, B, T)
    assert np.array_equal(d2, d) and np.array_equal(x2, x)
    nb, odd, lane, s = H // 32 - 1, 1, 27, 5
    u16 = dump.view(np.uint16).reshape(B, T, L, 2, H // 32, 2, 64, 8)
    for which, src in ((0, d), (1, x)):
        want = src[l, b, DL.dump16_feature(nb, lane >> 4, s), 32 * t + 16 * odd + (lane & 15)]
        assert DL.bf16_to_f32(u16[b, t, l, which, nb, odd, lane, s]) == want
    # an even slot is the low half of its 32-bit word
    w32 = dump.view(np.uint32).reshape(B, T, L, 2, H // 32, 2, 64, 4)[b, t, l, 0, nb, odd, lane]
    assert (w32[2] & 0xFFFF) == u16[b, t, l, 0, nb, odd, lane, 4] and (w32[2] >> 16) == u16[b, t, l, 0, nb, odd, lane, 5]

    codes = rng.integers(0, 65536, size=(L, B, H, 32 * T)).astype(np.uint16)
    tape = DL.encode_tape16(codes)
    assert tape.dtype == np.float32 and tape.size * 2 == codes.size                       # H * 64 bytes per block
    assert np.array_equal(DL.decode_tape16(tape, L, H, B, T), codes)
    assert tape.view(np.uint16).reshape(B, T, L, H // 32, 2, 64, 8)[b, t, l, nb, odd, lane, s] == \
        codes[l, b, DL.dump16_feature(nb, lane >> 4, s), 32 * t + 16 * odd + (lane & 15)]


def test_bf16_rounds_to_nearest_even_and_decodes_by_a_shift():
    f = lambda bits: np.array([bits], np.uint32).view(np.float32)
    assert DL.bf16_round(f(0x3F808000))[0] == 0x3F80          # a tie: down to the even code
    assert DL.bf16_round(f(0x3F818000))[0] == 0x3F82          # a tie: up to the even code
    assert DL.bf16_round(f(0x3F808001))[0] == 0x3F81
    assert DL.bf16_round(f(0x3F807FFF))[0] == 0x3F80
    assert DL.bf16_round(f(0x7F7FFFFF))[0] == 0x7F80          # rounds over to Inf, as the hardware conversion does
    assert np.isnan(DL.bf16_to_f32(DL.bf16_round(np.array([np.nan], np.float32))))[0]
    assert DL.bf16_to_f32(np.array([0xC0A0], np.uint16))[0] == -5.0
    m = np.arange(-128, 129, dtype=np.float32) / 128          # the synthetic operands of the GPU test: exact in bf16
    assert np.array_equal(DL.bf16_to_f32(DL.bf16_round(m)), m)


def test_tape16_codes():
    th = np.array([0.0, 0.25, -0.25, 3.5, 1 - 2.0 ** -18, 0.5 / 65536, 1.5 / 65536, np.inf, -np.inf, np.nan, 65535.2 / 65536, 65534.6 / 65536],
                  np.float32)
    want = [0, 16384, 49152, 32768, 0, 0, 2, 0xFFFF, 0xFFFF, 0xFFFF, 0, 0xFFFE]        # a finite phase never takes the reserved code
    assert DL.tape16_code(th).tolist() == want
    ph = DL.tape16_phase(np.array([0, 1, 0x8000, 0xFFFE, 0xFFFF], np.uint16))
    assert ph[:4].tolist() == [0.0, 1 / 65536, 0.5, 65534 / 65536] and np.isnan(ph[4])
    codes = np.arange(0xFFFF, dtype=np.uint16)                # every finite code is a fixed point of decode -> encode
    assert np.array_equal(DL.tape16_code(DL.tape16_phase(codes)), codes)


# ---- tests/wgrad_cases.py: what can be checked without a device -------------------------------------------------------
def test_case_table_covers_the_chunk_edges_on_the_assumed_device():
    cov = WC.coverage(WC.DEVICE_CUS)
    WC.assert_coverage(cov)
    assert len({c.id for c in WC.CASES}) == len(WC.CASES)
    for c in WC.CASES:
        assert c.P % 32 == 0 and (c.B * c.P <= 2 * 1056 if c.H == 256 else c.B * c.P <= 9600)


def test_planners_on_the_documented_cases():
    """the 300-tile case on 256 CUs (thin jobs: 256 chunks of 2 tiles, 106 empty; FiLM gather: 64 chunks of 5, 4 empty) and the planners' edges"""
    assert WC.wgrad_nchunk_thin(9, 1, 300, 256) == 256 and -(-300 // 256) == 2
    assert sum(1 for k in range(256) if k * 2 >= 300) == 106
    assert WC.film_nchunk(300) == 64 and sum(1 for k in range(64) if k * 5 >= 300) == 4
    assert WC.wgrad_nchunk(9, 1, 1, 256) == 1 and WC.wgrad_nchunk_thin(9, 2, 1, 256) == 1 and WC.film_nchunk(1) == 1
    assert WC.wgrad_nchunk_thin(9, 2, 1000, 8) == 8 and WC.wgrad_nchunk_thin(9, 1, 1000, 256) == 256
    assert WC.chunk_lengths(7, 3) == [3, 3, 1] and WC.chunk_lengths(5, 4) == [2, 2, 1, 0] and WC.chunk_lengths(300, 64)[59:] == [5, 0, 0, 0, 0]


@pytest.mark.parametrize("case", [c for c in WC.CASES if c.T in (1, 5, 33) and c.B == 2 and c.cus == 0], ids=lambda c: c.id)
def test_tile_sensitivity_condition_holds_on_a_synthetic_reference(case):
    """the condition of the GPU test, on operands with the GPU test's statistics (d theta normal, x a sine): removing any one tile moves
    some element of every square dW by more than twice the bound -- and the helper does notice a tile whose operands vanish"""
    rng = np.random.default_rng(5)
    L, B, H, P = 3, case.B, case.H, case.P
    dth = rng.normal(size=(L, B, H, P))
    x = np.sin(rng.uniform(-3, 3, size=(L, B, H, P)))
    freq = rng.uniform(20, 40, size=(B, L, H))
    for l in range(1, L):
        terms = WC.square_tile_terms(dth[l], x[l - 1], freq[:, l])            # [B, T, H, H]
        ref = terms.sum((0, 1))
        bound = WC.bound(e32=2.0 ** -22 * np.abs(ref).max(), c=2.0 ** -15, mag=WC.square_magnitude(dth[l], x[l - 1], freq[:, l]), ref=ref, factor=4)
        assert WC.insensitive_tiles(terms, bound) == []
        terms[B - 1, case.T - 1] *= 1e-9
        assert WC.insensitive_tiles(terms, bound) == [(B - 1, case.T - 1)]


@pytest.mark.parametrize("route", WC.ROUTES, ids=lambda r: r.name)
@pytest.mark.parametrize("kind", ["texture", "baseline"])
def test_reference_on_encoded_operands_is_the_plain_contraction(kind, route):
    """WC.reference on buffers made by the encoders: the tensors it returns for the route, and one square and one thin weight gradient and
    the phase sums against an einsum written out here -- the decoding, the FiLM preparation and the operand choice of every route"""
    case = WC.Case(kind, 32, 3, 2, 0)
    sp, sd, inp = WC.spec_of(case), WC.state_dict(kind, 32), WC.inputs(kind, 32, 3, 2)
    H, ng, nc, G, C = 32, sp["n_geo"], sp["n_color"], sp["grid_ch"], sp["output_dim"]
    L, B, P = ng + nc, case.B, case.P
    rng = np.random.default_rng(11)
    dth = rng.normal(size=(L, B, H, P)).astype(np.float32)
    acc = rng.normal(size=(L, B, H, P)).astype(np.float32)                   # the fp32 tape: raw accumulators
    codes = rng.integers(0, 0xFFFF, size=(L, B, H, P)).astype(np.uint16)
    fp, pp, inv, freq = WC.film_prepared(sd, sp, inp["film"], route.precision == "f16x3")
    assert (inv[0] == 1).all() and ((inv[1:] == 1).all() if route.precision == "f32" else (np.log2(inv[1:]) % 1 == 0).all())
    if route.tape_format == WC.TAPE_U16:
        tape, x_tape = DL.encode_tape16(codes), np.sin(2 * np.pi * codes.astype(np.float64) / 65536)
    else:
        arg = fp.transpose(1, 0, 2)[..., None].astype(np.float64) * acc + pp.transpose(1, 0, 2)[..., None]
        tape, x_tape = DL.encode_f32_dump(acc), np.sin(2 * np.pi * arg)
    if route.amp:
        x_sq = DL.bf16_to_f32(DL.bf16_round(np.cos(acc)))
        dth = DL.bf16_to_f32(DL.bf16_round(dth))
        d_t = DL.encode_bf16_dump(dth, x_sq)
    else:
        x_sq, d_t = x_tape, DL.encode_f32_dump(dth)
    bufs = dict(tape=tape, d_t=np.concatenate([d_t, np.full(64, np.nan, np.float32)]), out=rng.random((B, P, C)).astype(np.float32),
                d_out=inp["d_out"], tape_e=rng.normal(size=(B * P, 32)).astype(np.float32) if G else None)
    ref = WC.reference(route, sp, sd, inp, bufs, d_phase_got=dth.sum(-1).transpose(1, 0, 2))
    want = {f"geo_w.{i}" for i in range(ng)} | {f"color_w.{i}" for i in range(1, nc)} | {"color_w.0.x", "color_w.0.side", "head_w", "head_b", "rgb_w", "rgb_b"}
    if not route.amp:
        want |= {f"geo_b.{i}" for i in range(ng)} | {f"color_b.{i}" for i in range(nc)} | {"d_phase_geo", "d_phase_app", "d_freq_geo", "d_freq_app"}
    elif route.tape_format != WC.TAPE_F32:
        want |= {"d_freq_geo", "d_freq_app"}
    assert set(ref) == want
    close = lambda a, b: np.abs(a - b).max() <= 1e-12 * np.abs(b).max()
    l = 3
    assert close(ref[f"geo_w.{l}"].ref, np.einsum("bn,bnp,bkp->nk", freq[:, l], dth[l].astype(np.float64), np.asarray(x_sq[l - 1], np.float64)))
    assert ref[f"geo_w.{l}"].c == route.c_square and ref[f"geo_w.{l}"].insensitive == [] and ref["geo_w.0"].c == 0
    warped = inp["points"].astype(np.float64) * float(np.float32(2 / 0.24))
    assert close(ref["geo_w.0"].ref, np.einsum("bn,bnp,bpk->nk", freq[:, 0], dth[0].astype(np.float64), warped))
    d_out = inp["d_out"].astype(np.float64)
    head = np.einsum("bpr,bkp->rk", np.concatenate([d_out[..., :C - 4], d_out[..., -1:]], -1), x_tape[ng - 1])
    assert close(ref["head_w"].ref[:C - 3], head) and not ref["head_w"].ref[C - 3:].any()
    assert close(ref["head_b"].ref[:C - 3], np.concatenate([d_out[..., :C - 4], d_out[..., -1:]], -1).sum((0, 1)))
    rgb = bufs["out"][..., C - 4:C - 1].astype(np.float64)
    assert close(ref["rgb_w"].ref, np.einsum("bpc,bkp->ck", d_out[..., C - 4:C - 1] * rgb * (1 - rgb), x_tape[L - 1]))
    side = np.concatenate([inp["dirs"].astype(np.float64)] + ([bufs["tape_e"].reshape(B, P, 32).astype(np.float64)] if G else []), -1)
    assert close(ref["color_w.0.side"].ref, np.einsum("bn,bnp,bpk->nk", freq[:, ng], dth[ng].astype(np.float64), side))
    if not route.amp:
        assert close(ref["d_phase_app"].ref, dth[ng:].astype(np.float64).sum(-1).transpose(1, 0, 2).reshape(B, -1))
        assert close(ref["geo_b.2"].ref, (freq[:, 2] * dth[2].astype(np.float64).sum(-1)).sum(0))
    if "d_freq_geo" in ref:
        W, b = WC.film_layers(sd, sp)
        z = np.einsum("nk,bkp->bnp", W[l].astype(np.float64), np.asarray(x_sq[l - 1], np.float64)) + b[l].astype(np.float64)[None, :, None]
        if route.tape_format == WC.TAPE_F32:
            z = acc[l].astype(np.float64) * inv[l].astype(np.float64)[None, :, None] + b[l].astype(np.float64)[None, :, None]
        assert close(ref["d_freq_geo"].ref.reshape(B, ng, H)[:, l], 15 * (dth[l].astype(np.float64) * z).sum(-1))
