"""The kept lists of the split coarse pass (fenerf_set_render_split) as the density launch's tile masks + one scan make them: a 16-bit
mask per 16-sample tile, the trunk output parked at the sample's own slot, and per image the ascending list of kept sample indices from
an exclusive prefix over the masks' popcounts (fenerf_split_scan).  Every render case asserts torch.equal between the split route and the
dense route on rgb, depth and weights; the scan is also held to numpy on masks of its own."""
import functools

import numpy as np
import pytest
import torch

from fenerf_amd import _lib, native, procedural as proc
from fenerf_amd.generators import volumetric_rendering as VR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KIND, H, GRID = "texture", 64, 8


def T(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float32), device=DEV)


@functools.lru_cache(maxsize=None)
def _state():
    spec = proc.model_spec(KIND, hidden_dim=H, grid_size=GRID, z_dim=8)
    return spec, proc.make_state_dict(spec, seed=6, sigma_gain=60.0, with_mapping=False)


def _model(shift=0.0):
    """the model with its sigma bias lowered by `shift`"""
    spec, sd = _state()
    sd = dict(sd)
    sd["final_layer.bias"] = sd["final_layer.bias"] - np.float32(shift)
    return native.NativeModel(sd, spec, DEV, "f16x3")


@functools.lru_cache(maxsize=None)
def _plain():
    return _model()


def _inputs(B, S, N, seed):
    spec, _ = _state()
    film = proc.film_params(spec, B, seed=seed)
    torch.manual_seed(12 + seed)
    o, d, z, _, _ = VR.sample_rays(B, N, DEV, 12, (S, S), 0.88, 1.12, 0.3, 0.155, np.pi / 2, np.pi / 2, "gaussian")
    u = torch.rand((B * S * S, N), device=DEV)
    return dict(o=o, d=d, z=z, u=u, film={k: T(film[k]) for k in ("freq_geo", "phase_geo", "freq_app", "phase_app")})


def _tf(a):
    return tuple(a["film"][k] for k in ("freq_geo", "phase_geo", "freq_app", "phase_app"))


def _sigma(nat, a):
    """[B, R N] sigma rows of the dense kernel"""
    B = a["z"].shape[0]
    return nat.siren_forward_rays(a["o"], a["d"], a["z"], *_tf(a))[..., -1].reshape(B, -1)


def _kept_mask(nat, a):
    return ~(_sigma(nat, a) <= 0)


def _kept(nat, a):
    return [int(v) for v in _kept_mask(nat, a).sum(1)]


def _render(nat, a, mode, timing=None):
    opts = _lib.composite_opts("relu", 0.0, fill_mode="seg_padding_background", fill_color="black")
    with native.render_split(mode), native.render_fusion("off"), native.phase_timing() as t:
        out = nat.render(a["o"], a["d"], a["z"], a["u"], None, None, *_tf(a), opts, hierarchical=True, want_weights=True, want_wsum=True)
        torch.cuda.synchronize()
    if timing is not None:
        timing.update(t.calls)
    return out[:3]


def _assert_equal(nat, a, what):
    calls = {}
    dense = [t.clone() for t in _render(nat, a, "off")]
    split = _render(nat, a, "force", timing=calls)
    assert calls.get("siren_density") == 1 and calls.get("siren_colour") == 1, calls
    for name, x, y in zip(("rgb", "depth", "weights"), dense, split):
        assert torch.equal(x, y), (what, name, float((x - y).abs().nan_to_num().max()))


def _quantile_shift(a, share):
    """the bias shift that keeps about `share` of the samples of inputs `a`"""
    return float(torch.quantile(_sigma(_plain(), a).flatten().float(), 1.0 - share))


def test_partial_last_unit_and_empty_tiles():
    """12^2 rays x 12 samples, B = 2: 1,728 samples = 13.5 units of 128 per image; a tenth of the samples kept, so that some tiles of 16
    write a mask of 0 between tiles that keep samples (the fp32 oracle on such rays: 19 to 24 of an image's 108 tiles)"""
    B, S, N = 2, 12, 12
    a = _inputs(B, S, N, 0)
    nat = _model(_quantile_shift(a, 0.1))
    keep = _kept_mask(nat, a)
    per_tile = keep.reshape(B, -1, 16).sum(-1)
    print(f"[lists] 12x12x12: kept {keep.sum(1).tolist()} of {S * S * N}, tiles with no kept sample {(per_tile == 0).sum(1).tolist()} of {per_tile.shape[1]}")
    assert bool((per_tile == 0).any()) and bool((per_tile > 0).any()) and bool(((per_tile > 0) & (per_tile < 16)).any())
    assert (S * S * N) % 128 != 0
    _assert_equal(nat, a, "12x12x12")


def test_ragged_images_take_one_launch_each():
    """10^2 x 7, B = 3: 700 samples per image are no multiple of 32 -- a density launch per image on its own masks and slots, and a last tile
    of 12 real samples and 4 phantom lanes whose mask bits stay 0"""
    B, S, N = 3, 10, 7
    a = _inputs(B, S, N, 0)
    nat = _model(_quantile_shift(a, 0.5))
    k = _kept(nat, a)
    print(f"[lists] 10x10x7: kept {k} of {S * S * N}")
    assert (S * S * N) % 32 != 0 and (S * S * N) % 16 != 0 and all(0 < c < S * S * N for c in k), k
    _assert_equal(nat, a, "10x10x7")
    # ... and with every sample kept: the phantom lanes of the last tile sit next to 12 set bits
    full = _model(-1e6)
    assert _kept(full, a) == [S * S * N] * B
    _assert_equal(full, a, "10x10x7-full")


def test_an_empty_image_beside_a_full_one():
    """One image with no kept sample beside one with every sample kept.  The sigma bias belongs to the model, not to the image, so what tells
    the images apart is their FiLM block: with the last trunk layer's frequency at 15 f + 30 = 0 an image's sigma is one constant, set by its
    phases; the bias goes between the two constants."""
    B, S, N = 2, 8, 6
    a = _inputs(B, S, N, 0)
    spec, _ = _state()
    fg = a["film"]["freq_geo"].clone()
    fg[:, (spec["n_geo"] - 1) * H:] = -2.0
    a["film"]["freq_geo"] = fg
    sig = _sigma(_plain(), a)
    lo, hi = sorted([(float(sig[b].min()), float(sig[b].max())) for b in range(B)])
    assert lo[1] < hi[0], (lo, hi)
    nat = _model(0.5 * (lo[1] + hi[0]))
    k = _kept(nat, a)
    print(f"[lists] empty beside full: sigma ranges {lo} {hi}, kept {k}")
    assert sorted(k) == [0, S * S * N], k
    _assert_equal(nat, a, "empty-beside-full")


@pytest.mark.parametrize("count", [1, 16, 17, 129])
def test_exact_kept_counts(count):
    """an image that keeps exactly `count` samples (one bit; one full tile's worth; one more; one more than a unit of 128): the first input
    seed whose sigma values leave a gap behind the count-th largest takes the bias into that gap"""
    B, S, N = 2, 8, 6
    chosen = None
    for seed in range(50):
        a = _inputs(B, S, N, seed)
        s = torch.sort(_sigma(_plain(), a)[0].float(), descending=True).values
        hi, lo = float(s[count - 1]), float(s[count])
        if hi - lo < 1e-3 * max(1.0, abs(hi)):
            continue
        nat = _model(0.5 * (hi + lo))
        k = _kept(nat, a)
        if k[0] == count:
            chosen = (seed, nat, a, k)
            break
    assert chosen is not None, f"no seed in 0..49 gives an image with exactly {count} kept samples"
    seed, nat, a, k = chosen
    print(f"[lists] count {count}: seed {seed}, kept {k}")
    _assert_equal(nat, a, f"count-{count}")


def test_second_render_with_fewer_kept_samples_is_its_own():
    """masks, lists and parked operands of an earlier, fuller render on the same workspace must not reach the next one"""
    B, S, N = 2, 8, 6
    a1, a2 = _inputs(B, S, N, 1), _inputs(B, S, N, 2)
    nat = _model(_quantile_shift(a1, 0.5))
    k1, k2 = _kept(nat, a1), _kept(nat, a2)
    if sum(k1) < sum(k2):
        a1, a2, k1, k2 = a2, a1, k2, k1
    print(f"[lists] second render: kept {k1} then {k2}")
    assert sum(k2) < sum(k1) and sum(k2) > 0, (k1, k2)
    dense2 = [t.clone() for t in _render(nat, a2, "off")]
    _render(nat, a1, "force")
    for name, x, y in zip(("rgb", "depth", "weights"), dense2, _render(nat, a2, "force")):
        assert torch.equal(x, y), ("second render", name)
    # ... nor an emptier one: after it, the fuller render is still its own
    dense1 = [t.clone() for t in _render(nat, a1, "off")]
    for name, x, y in zip(("rgb", "depth", "weights"), dense1, _render(nat, a1, "force")):
        assert torch.equal(x, y), ("third render", name)


def test_lists_across_scan_workgroups():
    """20^2 rays x 12 samples, B = 2: 4,800 samples = 300 tiles per image, so an image's list is written by two scan workgroups (256 tiles
    each) and the second one's entries start at the count of the first one's tiles; kept samples on both sides of sample 4,096"""
    B, S, N = 2, 20, 12
    a = _inputs(B, S, N, 0)
    nat = _model(_quantile_shift(a, 0.3))
    keep = _kept_mask(nat, a)
    first, second = keep[:, :4096].sum(1).tolist(), keep[:, 4096:].sum(1).tolist()
    print(f"[lists] 20x20x12: kept {first} in tiles 0..255, {second} in tiles 256..299")
    assert S * S * N > 4096 and all(c > 0 for c in first + second), (first, second)
    _assert_equal(nat, a, "20x20x12")


@pytest.mark.parametrize("tiles", [1, 37, 255, 256, 257, 513, 9001])
def test_scan_against_numpy(tiles):
    """fenerf_split_scan on masks of its own: random dense, random sparse, all-zero and all-ones images side by side.  A scan workgroup
    takes 256 tiles and counts the tiles before its own itself: one partial workgroup, one short of a full one, exactly one, one tile
    into a second, one tile into a third, and 36 workgroups (a prefix pass of more than one stride)"""
    rng = np.random.default_rng(tiles)
    m = np.stack([rng.integers(0, 65536, tiles), rng.integers(0, 65536, tiles) & rng.integers(0, 65536, tiles) & rng.integers(0, 65536, tiles),
                  np.zeros(tiles, np.int64), np.full(tiles, 65535), rng.integers(0, 65536, tiles) * (rng.random(tiles) < 0.1)]).astype(np.uint16)
    idx, counts = native.split_scan(torch.from_numpy(m.view(np.int16)).to(DEV))
    torch.cuda.synchronize()
    idx, counts = idx.cpu().numpy(), counts.cpu().numpy()
    bits = ((m[:, :, None] >> np.arange(16, dtype=np.uint16)) & 1).reshape(m.shape[0], -1).astype(bool)
    assert counts.tolist() == bits.sum(1).tolist()
    assert counts[2] == 0 and counts[3] == 16 * tiles
    for b in range(m.shape[0]):
        assert np.array_equal(idx[b, :counts[b]], np.flatnonzero(bits[b]).astype(np.int32)), b
        assert (idx[b, counts[b]:] == -1).all(), (b, "entries behind the list are not written")
