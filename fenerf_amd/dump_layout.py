"""numpy encode / decode of the backward's dump formats (csrc/fenerf_layout.h "Tape", "bf16 dump", "16-bit tape"): what the forward-save
and chain kernels leave for the weight-gradient kernels (csrc/fenerf_siren_wgrad.hip), readable from Python.  Pure numpy, no device.

Every decoded array is [layer][image][feature][point]; every encoder takes that shape and returns the flat buffer of one call over
B images of 32 * tiles_per_image points each (global tile = image * tiles_per_image + t).  The per-tile FiLM sums that the chain
kernels append to the d(theta) dump are NOT described here: they stay opaque.

    fp32 register dump (tape, d theta)   [tile][layer][g = H/8][lane 64][4 x f32]
        element i of lane (m = lane & 31, half = lane >> 5): feature tape_feature(g, half, i) of point 32 tile + m
    bf16 dump, a (tile32, layer) block of H * 128 bytes   [d theta | x][nb = H/32][16-point tile 2][lane 64][8 x bf16]
        slot t of lane (n = lane & 15, g = lane >> 4): feature dump16_feature(nb, g, t) of point 32 tile + 16 odd + n;
        an even slot is the low half of its 32-bit word (little endian: slot t is the t-th 16-bit value of the piece)
    16-bit tape, a block of H * 64 bytes   [nb][16-point tile 2][lane 64][8 x u16], the same pieces; code = frac(theta) * 65536
"""
import numpy as np

WIDTHS = (32, 64, 96, 128, 192, 256)      # the instantiated hidden widths
TAPE16_NONFINITE = 0xFFFF


def tape_feature(g, half, i):
    return 32 * (g >> 2) + 8 * (g & 3) + 4 * half + i


def dump16_feature(nb, g, t):
    return 32 * nb + 16 * (g >> 1) + 4 * (g & 1) + 8 * (t >> 2) + (t & 3)


def f32_dump_index(H):
    """-> (feature, point in the 32-point tile) of every float of a (tile, layer) block, in storage order: two int arrays [H * 32]"""
    g, lane, i = np.meshgrid(np.arange(H // 8), np.arange(64), np.arange(4), indexing="ij")
    return tape_feature(g, lane >> 5, i).reshape(-1), (lane & 31).reshape(-1)


def dump16_index(H):
    """-> (feature, point in the 32-point tile) of every 16-bit value of one operand of a (tile32, layer) block: two int arrays [H * 32]"""
    nb, odd, lane, t = np.meshgrid(np.arange(H // 32), np.arange(2), np.arange(64), np.arange(8), indexing="ij")
    return dump16_feature(nb, lane >> 4, t).reshape(-1), (16 * odd + (lane & 15)).reshape(-1)


def _scatter(blocks, feat, pt, H):
    """blocks [B, T, L, H * 32] in storage order -> [L, B, H, 32 T]"""
    B, T, L, _ = blocks.shape
    out = np.empty((L, B, T, H, 32), blocks.dtype)
    out[..., feat, pt] = blocks.transpose(2, 0, 1, 3)
    return np.ascontiguousarray(out.transpose(0, 1, 3, 2, 4)).reshape(L, B, H, T * 32)


def _gather(vals, feat, pt):
    """[L, B, H, 32 T] -> blocks [B, T, L, H * 32] in storage order"""
    L, B, H, P = vals.shape
    v = vals.reshape(L, B, H, P // 32, 32).transpose(0, 1, 3, 2, 4)[..., feat, pt]          # [L, B, T, H * 32]
    return np.ascontiguousarray(v.transpose(1, 2, 0, 3))


# ---- fp32 register dump ---------------------------------------------------------------------------
def f32_dump_floats(L, H, B, tiles_per_image):
    return B * tiles_per_image * L * H * 32


def decode_f32_dump(buf, L, H, B, tiles_per_image):
    """flat float32 buffer (anything behind the dump is ignored) -> float32 [L, B, H, P]"""
    n = f32_dump_floats(L, H, B, tiles_per_image)
    blocks = np.asarray(buf, dtype=np.float32).reshape(-1)[:n].reshape(B, tiles_per_image, L, H * 32)
    return _scatter(blocks, *f32_dump_index(H), H)


def encode_f32_dump(vals):
    """float32 [L, B, H, P] -> the flat float32 dump"""
    vals = np.asarray(vals, dtype=np.float32)
    return _gather(vals, *f32_dump_index(vals.shape[2])).reshape(-1)


# ---- bf16 <-> fp32 ----------------------------------------------------------------------------------
def bf16_round(x):
    """float32 -> bf16 bits (uint16), round to nearest even; NaN stays a (quiet) NaN"""
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = np.isnan(np.asarray(x, dtype=np.float32))
    return np.where(nan, np.uint16(0x7FC0), r)


def bf16_to_f32(bits):
    """bf16 bits -> float32: a shift"""
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


# ---- bf16 dump ----------------------------------------------------------------------------------------
def decode_bf16_dump(buf, L, H, B, tiles_per_image):
    """flat buffer (float32 words or bytes, as the chain kernel wrote it; the FiLM sums behind it are ignored)
    -> (d theta, x): float32 [L, B, H, P] each.  x of the last layer is not written by the kernels: whatever the block holds."""
    u = np.ascontiguousarray(buf).reshape(-1).view(np.uint16)[: B * tiles_per_image * L * H * 64]
    blocks = u.reshape(B, tiles_per_image, L, 2, H * 32)
    feat, pt = dump16_index(H)
    return tuple(bf16_to_f32(_scatter(np.ascontiguousarray(blocks[:, :, :, w]), feat, pt, H)) for w in (0, 1))


def encode_bf16_dump(d_theta, x):
    """float32 [L, B, H, P] twice -> the flat dump as float32 words (H * 32 words per block, like the fp32 dump)"""
    d_theta, x = np.asarray(d_theta, dtype=np.float32), np.asarray(x, dtype=np.float32)
    feat, pt = dump16_index(d_theta.shape[2])
    halves = [_gather(bf16_round(v), feat, pt) for v in (d_theta, x)]                   # [B, T, L, H * 32] u16 each
    return np.ascontiguousarray(np.stack(halves, axis=3)).reshape(-1).view(np.float32)


# ---- 16-bit tape --------------------------------------------------------------------------------------
def tape16_code(theta):
    """phase in revolutions (float32) -> code: frac(theta) * 65536 rounded to nearest even, 65536 wraps to 0; not finite -> 0xffff; a
    finite phase that would round to 0xffff is stored as 0xfffe (from below) or 0 (phase_u16, csrc/fenerf_siren_f16w.hip)"""
    theta = np.asarray(theta, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        v = (theta - np.floor(theta)).astype(np.float32) * np.float32(65536)
        c = (np.rint(np.where(np.isfinite(v), v, 0)).astype(np.int64) & 0xFFFF).astype(np.uint16)
        c = np.where(c == TAPE16_NONFINITE, np.where(v < 65535, np.uint16(0xFFFE), np.uint16(0)), c)
    return np.where(np.isfinite(theta), c, np.uint16(TAPE16_NONFINITE)).astype(np.uint16)


def tape16_phase(code):
    """code -> frac(theta) in revolutions (float32, exact); 0xffff -> NaN (tape16_phase, csrc/fenerf_trig.h)"""
    code = np.asarray(code, dtype=np.uint16)
    return np.where(code == TAPE16_NONFINITE, np.float32(np.nan), code.astype(np.float32) * np.float32(1 / 65536)).astype(np.float32)


def decode_tape16(buf, L, H, B, tiles_per_image):
    """flat buffer (float32 words or bytes) -> codes uint16 [L, B, H, P]"""
    u = np.ascontiguousarray(buf).reshape(-1).view(np.uint16)[: B * tiles_per_image * L * H * 32]
    return _scatter(u.reshape(B, tiles_per_image, L, H * 32), *dump16_index(H), H)


def encode_tape16(codes):
    """codes uint16 [L, B, H, P] -> the flat tape as float32 words (two codes per word)"""
    codes = np.asarray(codes, dtype=np.uint16)
    return _gather(codes, *dump16_index(codes.shape[2])).reshape(-1).view(np.float32)
