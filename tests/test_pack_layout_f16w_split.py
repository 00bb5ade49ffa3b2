"""CPU check of the split coarse pass of fenerf_siren_f16w.hip (PASS = 1 density, PASS = 2 colour) on the packer's real stream: a numpy
wave walks the stream the way the kernel's prefetch pointer does -- FENERF_DPF chunks ahead of the consumer, with the jumps of g_next over
the stages a pass does not run placed where the kernel places them (at step `stage chunks - DPF` of the stage before the gap) -- along the
density path (layer 0, trunk, label / sigma head) and the colour path (colour layer 0 from the parked trunk output, colour layers, rgb
head), and reproduces the fp64 oracle's labels / sigma and rgb.  A jump in the wrong step or to the wrong chunk feeds a stage another
stage's weights.  The full-path emulation of tests/test_pack_layout_f16w.py runs on the same (unchanged) stream."""
import numpy as np
import pytest

from fenerf_amd import _lib, procedural as proc
from oracle import fenerf_oracle as O
from test_pack_layout_f16 import split16
from test_pack_layout_f16w import CH, DPF, G_, N_, NSLOT, dma_operand, mfma16w, mfma32w, row_of


class Walk:
    """the prefetch pointer of one tile: DPF chunks of the pass's first stage are in flight when the tile starts"""

    def __init__(self, ring, first):
        self.ring, self.first, self.g_next, self.fifo = ring, first, first, []
        for _ in range(DPF):
            self.issue()

    def issue(self):
        assert 0 <= self.g_next < self.ring.shape[0] - DPF, "a prefetch past the tile's stream"
        self.fifo.append(self.g_next)
        self.g_next += 1

    def stage(self, n_chunks, jump_by=0, jump_to=None):
        """chunk steps of one stage: at step n_chunks - DPF the pointer leaves for the stage the pass runs next"""
        assert n_chunks % NSLOT == 0 and n_chunks >= DPF
        for i in range(n_chunks):
            if i == n_chunks - DPF:
                self.g_next = self.g_next + jump_by if jump_to is None else jump_to
            self.issue()
            yield self.ring[self.fifo.pop(0)]


def _setup(kind, H, grid):
    spec = proc.model_spec(kind, hidden_dim=H, grid_size=grid, z_dim=8)
    sd = proc.make_state_dict(spec, seed=12, sigma_gain=500.0, with_mapping=False)
    blob, consts = _lib.pack_weights_host(sd, spec, "f16x3")
    rng = np.random.default_rng(1)
    pts = rng.uniform(-0.13, 0.13, (16, 3)).astype(np.float32)
    dirs = rng.normal(size=(16, 3)).astype(np.float32)
    dirs /= np.linalg.norm(dirs, axis=-1, keepdims=True)
    film = proc.film_params(spec, 1, seed=12)
    grid_cl = np.ascontiguousarray(sd["spatial_embeddings"][0].transpose(1, 2, 3, 0)).astype(np.float64) if grid else None
    return spec, sd, blob, consts, pts, dirs, film, grid_cl


def emulate_split(blob, consts, spec, pts, dirs, film, grid_cl):
    H, NB, KS = spec["hidden_dim"], spec["hidden_dim"] // 32, spec["hidden_dim"] // 32
    has_grid = spec["grid_ch"] > 0
    QB = (KS + 1) // 2
    C0_QB = (2 * (2 * KS + (2 if has_grid else 0) + 1) + CH - 1) // CH
    pad = lambda chunks: (chunks + NSLOT - 1) // NSLOT * NSLOT
    SQ, C0, HEAD = pad(NB * QB), pad(NB * C0_QB), pad(QB)
    n_geo, n_color, C = spec["n_geo"], spec["n_color"], spec["output_dim"]
    n_lab, L = C - 4, n_geo + n_color
    l0 = blob[:NB * 256].astype(np.float64)
    ring = blob[NB * 256:].view(np.float16).reshape(-1, CH, 64, 8).astype(np.float64)
    assert ring.shape[0] == (n_geo - 1) * SQ + C0 + HEAD + (n_color - 1) * SQ + HEAD + DPF       # the stream did not grow
    c0_off = (n_geo - 1) * SQ

    fg = film["freq_geo"][0].astype(np.float32) * np.float32(15) + np.float32(30)
    fa = film["freq_app"][0].astype(np.float32) * np.float32(15) + np.float32(30)
    f_all = np.concatenate([fg, fa]).astype(np.float64).reshape(L, H)
    p_all = np.concatenate([film["phase_geo"][0], film["phase_app"][0]]).astype(np.float64).reshape(L, H)
    bias = consts[36:36 + L * H].astype(np.float64).reshape(L, H)
    inv = consts[36 + L * H:36 + 2 * L * H].astype(np.float64).reshape(L, H)
    head_inv = consts[36 + 2 * L * H:36 + 2 * L * H + 32].astype(np.float64)
    rgb_inv = consts[36 + 2 * L * H + 32:36 + 2 * L * H + 36].astype(np.float64)
    fp, pp = f_all / (2 * np.pi) * inv, (f_all * bias + p_all) / (2 * np.pi)
    q = pts[N_].astype(np.float64) * (2 / 0.24)
    d = dirs[N_].astype(np.float64)
    feat0 = 16 * (G_ >> 1) + 4 * (G_ & 1)

    def film_pack(acc, layer, nb):
        hi = np.zeros((64, 8)); lo = np.zeros((64, 8))
        for rt in range(2):
            feat = 32 * nb + feat0[:, None] + 8 * rt + np.arange(4)[None, :]
            v = 16 * np.sin(2 * np.pi * (fp[layer][feat] * acc[rt] + pp[layer][feat]))
            hi[:, 4 * rt:4 * rt + 4], lo[:, 4 * rt:4 * rt + 4] = split16(v)
        return hi, lo

    def run_stage(chunks, bops, qb, n_bodies):
        """n_bodies n-block bodies of qb chunks, then the stage's padding chunks (zero weights) -> acc[body][rt]"""
        accs = []
        for _ in range(n_bodies):
            acc = [np.zeros((64, 4)), np.zeros((64, 4))]
            for qc in range(qb):
                chunk = next(chunks)
                for spl in range(2):
                    sp = 2 * qc + spl
                    if sp < len(bops):
                        bh, bl = bops[sp]
                        for rt in range(2):
                            ahi, alo = dma_operand(chunk, spl, rt, 0), dma_operand(chunk, spl, rt, 1)
                            mfma16w(alo, bh, acc[rt]); mfma16w(ahi, bl, acc[rt]); mfma16w(ahi, bh, acc[rt])
                    else:
                        assert not chunk[4 * spl:4 * spl + 4].any()
            accs.append(acc)
        for chunk in chunks:
            assert not chunk.any()
        return accs

    out = np.zeros((16, C))
    # ---------------- density path: layer 0, G1 .. G(n_geo-1) with the jump over colour layer 0, the head ----------------
    b0 = np.select([G_ == 0, G_ == 1, G_ == 2], [q[:, 0], q[:, 1], q[:, 2]], 0.0)
    x = []
    for nb in range(NB):
        acc = [np.zeros((64, 4)), np.zeros((64, 4))]
        for rt in range(2):
            a0 = np.array([l0[nb * 256 + ((G_[l] & 1) * 32 + row_of(rt, N_[l])) * 4 + (G_[l] >> 1)] for l in range(64)])
            mfma32w(a0, b0, acc[rt])
        x.append(film_pack(acc, 0, nb))
    first = 0 if n_geo > 1 else c0_off + C0
    w = Walk(ring, first)
    for l in range(1, n_geo):
        accs = run_stage(w.stage(SQ, jump_by=C0 if l == n_geo - 1 else 0), x, QB, NB)
        x = [film_pack(accs[nb], l, nb) for nb in range(NB)]
    acc = run_stage(w.stage(HEAD, jump_to=first), x, QB, 1)[0]
    assert w.fifo == list(range(first, first + DPF)), "the tile ends with the next tile's first chunks in flight"
    for rt in range(2):
        for r in range(4):
            row = feat0 + 8 * rt + r
            for l in range(64):
                if row[l] <= n_lab:
                    out[N_[l], row[l] if row[l] < n_lab else C - 1] = acc[rt][l, r] * head_inv[row[l]] + consts[row[l]]
    trunk = x           # what the density pass parks per kept point: the (hi, lo) B operands of colour layer 0, k32-step by k32-step

    # ---------------- colour path: colour layer 0 from the parked operands, the jump over the head, C1 .., the rgb head ----------------
    e = np.zeros((64, 8))
    if has_grid:
        Dg, Hg, Wg = grid_cl.shape[:3]
        ix, iy, iz = (q[:, 0] + 1) / 2 * (Wg - 1), (q[:, 1] + 1) / 2 * (Hg - 1), (q[:, 2] + 1) / 2 * (Dg - 1)
        x0, y0, z0 = np.floor(ix), np.floor(iy), np.floor(iz)
        ch0 = 16 * (G_ & 1) + 8 * (G_ >> 1)
        for c in range(8):
            cz, cy, cx = c >> 2, (c >> 1) & 1, c & 1
            xi, yi, zi = x0 + cx, y0 + cy, z0 + cz
            wgt = (ix - x0 if cx else x0 + 1 - ix) * (iy - y0 if cy else y0 + 1 - iy) * (iz - z0 if cz else z0 + 1 - iz)
            ok = (xi >= 0) & (xi <= Wg - 1) & (yi >= 0) & (yi <= Hg - 1) & (zi >= 0) & (zi <= Dg - 1)
            for l in range(64):
                if ok[l]:
                    e[l] += grid_cl[int(zi[l]), int(yi[l]), int(xi[l]), ch0[l]:ch0[l] + 8] * wgt[l]
    dv = np.zeros((64, 8)); dv[G_ == 0, :3] = d[G_ == 0] * 16
    bops = list(trunk) + ([split16(e * 16)] if has_grid else []) + [split16(dv)]
    w = Walk(ring, c0_off)
    accs = run_stage(w.stage(C0, jump_by=HEAD), bops, C0_QB, NB)
    x = [film_pack(accs[nb], n_geo, nb) for nb in range(NB)]
    for c in range(1, n_color):
        accs = run_stage(w.stage(SQ), x, QB, NB)
        x = [film_pack(accs[nb], n_geo + c, nb) for nb in range(NB)]
    acc = run_stage(w.stage(HEAD, jump_to=c0_off), x, QB, 1)[0]
    assert w.fifo == list(range(c0_off, c0_off + DPF))
    for r in range(3):
        for l in range(16):
            out[l, C - 4 + r] = 1 / (1 + np.exp(-(acc[0][l, r] * rgb_inv[r] + consts[32 + r])))
    return out


@pytest.mark.parametrize("kind,H,grid", [("texture", 32, 5), ("baseline", 32, 0), ("texture", 96, 5), ("texture", 256, 6)])
def test_density_and_colour_paths_on_the_packed_stream(kind, H, grid):
    spec, sd, blob, consts, pts, dirs, film, grid_cl = _setup(kind, H, grid)
    got = emulate_split(blob, consts, spec, pts, dirs, film, grid_cl)
    ref = O.siren_forward(sd, spec, pts[None], dirs[None], film["freq_geo"], film["phase_geo"], film["freq_app"], film["phase_app"],
                          dtype=np.float64)[0]
    np.testing.assert_allclose(got[..., :-1], ref[..., :-1], atol=3e-6, rtol=1e-5)
    np.testing.assert_allclose(got[..., -1], ref[..., -1], atol=1e-5 * max(1.0, np.abs(ref[..., -1]).max()), rtol=1e-5)


def test_full_path_emulation_still_walks_the_same_stream():
    from test_pack_layout_f16w import emulate_tile_f16w
    spec, sd, blob, consts, pts, dirs, film, grid_cl = _setup("texture", 32, 5)
    np.testing.assert_allclose(emulate_tile_f16w(blob, consts, spec, pts, dirs, film, grid_cl),
                               emulate_split(blob, consts, spec, pts, dirs, film, grid_cl), atol=1e-12, rtol=0)
