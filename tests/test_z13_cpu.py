"""The exact 13-bit weight image "z13" on the CPU (tests/z13_ref.py, the restatement the GPU tests hold the packer and the kernel to):
every bf16 bit pattern survives pack -> unpack wherever its block is not flagged, a block is flagged exactly when it holds a weight
the format cannot code, and on N(0, 0.02^2) weights almost no block is."""
import numpy as np
import torch

import z13_ref as z

K = 1024


def _all_patterns_matrix():
    """[640 + 64, 1024] uint16 holding every bf16 bit pattern, laid out so that pairs of 16-row tiles (32 rows) are
      rows   0..63   WIDE: the patterns in field order, 4 exponent fields per row, 128 fields per pair - most of them uncodable
      rows  64..575  NARROW: field f fills rows 64 + 2f, 65 + 2f (its 256 sign / mantissa patterns, 8 times): 16 fields per pair, all
                     codable but 255; the first of these pairs has base 15 and holds +-0 and every subnormal
      rows 576..703  four hand-made pairs of field-120 values with ONE planted weight each, in the second 512-k block only"""
    pat = np.arange(65536, dtype=np.uint32)
    by_field = (((pat >> 8) & 0xFF) << 7 | ((pat >> 7) & 1) << 15 | (pat & 0x7F)).astype(np.uint16)       # field-major order
    wide = by_field.reshape(64, K)
    narrow = np.repeat(by_field.reshape(256, 1, 256), 2, axis=1)            # [field, 2 rows, 256]
    narrow = np.tile(narrow, (1, 1, 4)).reshape(512, K)
    hand = np.tile(by_field[120 * 256:121 * 256], (128, 4)).copy()
    planted = {"nan": 0x7FC1, "-inf": 0xFF80, "2^-40 below": (120 - 40) << 7 | 0x15, "-0": 0x8000}
    for i, v in enumerate(planted.values()):
        hand[32 * i + 5, 700] = v
    return np.concatenate([wide, narrow, hand]), planted


def _field(w):
    return (w.astype(np.int64) >> 7) & 0xFF


def test_every_bf16_bit_pattern():
    w, planted = _all_patterns_matrix()
    N = w.shape[0]
    assert np.unique(w).size == 65536
    img = z.bf16_image(w)
    flags, bases, rec, flagged = z.pack(img, N)
    NP = N // 32
    # the image survives its byte form
    f2, b2, r2 = z.split_bytes(z.to_bytes(flags, bases, rec), N, K)
    assert np.array_equal(f2, flags) and np.array_equal(b2, bases) and np.array_equal(r2, rec)
    # expected bases and flags, straight from the definition, per pair and 512-k block
    wp = w.reshape(NP, 32, 2, 512)
    fld = _field(wp)
    want_base = np.where(fld != 255, fld, 0).max(axis=(1, 2, 3))
    assert np.array_equal(bases, want_base.astype(np.uint8))
    uncodable = (fld == 255) | (want_base[:, None, None, None] - fld > 30)
    want_flag = uncodable.any(axis=(1, 3))
    assert np.array_equal(flagged, want_flag)
    assert np.array_equal(flags, (want_flag[:, 0].astype(np.uint64) | want_flag[:, 1].astype(np.uint64) << np.uint64(1)))
    assert want_flag.any() and not want_flag.all()
    # round trip wherever the block is not flagged
    back = z.unpack(bases, rec, N // 16)
    keep = ~z.block_mask(flagged, N // 16, K // 32)
    assert np.array_equal(np.where(keep, back, 0), np.where(keep, img, 0))
    # by name.  The first narrow pair (rows 64..95: fields 0..15, base 15) codes +-0 and every subnormal, unflagged:
    p0 = 64 // 32
    assert bases[p0] == 15 and not flagged[p0].any()
    sub = w[64:66]
    assert {0x0000, 0x8000} <= set(sub.ravel().tolist()) and np.unique(sub).size == 256 and (_field(sub) == 0).all()
    tiles = slice(64 // 16, 96 // 16)
    assert np.array_equal(back[tiles], img[tiles])
    # the last narrow pair holds field 255 - Inf and every NaN payload, both signs: all of its blocks flag, its base is 254
    pl = (64 + 2 * 240) // 32
    assert bases[pl] == 254 and flagged[pl].all()
    nanrows = w[64 + 2 * 255:64 + 2 * 255 + 2]
    assert np.unique(nanrows).size == 256 and (_field(nanrows) == 255).all()
    # every block that holds an Inf / NaN anywhere is flagged
    assert flagged[(fld == 255).any(axis=(1, 3))].all()
    # the planted weights flag the second block of their pair and only that one; -0 among field-120 values is 120 below the base
    for i, name in enumerate(planted):
        p = 576 // 32 + i
        assert bases[p] == 120, name
        assert list(flagged[p]) == [False, True], name


def test_rows_beyond_n_and_the_missing_tile_never_flag():
    g = np.random.default_rng(5)
    N = 40                                                  # 3 tiles: pair 1 has one tile, whose rows 8..15 do not exist
    w = ((120 + g.integers(0, 8, (N, 128))) << 7 | g.integers(0, 128, (N, 128)) | g.integers(0, 2, (N, 128)) << 15).astype(np.uint16)
    img = z.bf16_image(w)
    flags, bases, rec, flagged = z.pack(img, N)
    assert not flagged.any() and flags.tolist() == [0, 0]
    back = z.unpack(bases, rec, 3)
    rows = np.arange(3)[:, None] * 16 + np.arange(64)[None, :] % 16
    exists = (rows < N)[:, None, :, None]
    assert np.array_equal(np.where(exists, back, 0), img)
    w[39, 70] = 0                                           # a zero in a row that exists does
    assert z.pack(z.bf16_image(w), N)[3].tolist() == [[False], [True]]


def test_fallback_share_on_normal_weights_is_capped():
    """N(0, 0.02^2) bf16, 2048 x 3584: the per-weight rate of values more than 30 binades below their pair's maximum is ~4e-8, about
    0.07 % of the (pair, 512-k) blocks; at most 1 % may flag - a packer that flags more has silently become the bf16 path."""
    w = (torch.randn(2048, 3584, generator=torch.Generator().manual_seed(0)) * 0.02).to(torch.bfloat16)
    bits = w.view(torch.int16).numpy().view(np.uint16)
    flagged = z.pack(z.bf16_image(bits), 2048)[3]
    assert flagged.shape == (64, 7)
    share = flagged.mean()
    print(f"flagged blocks: {int(flagged.sum())} of {flagged.size} ({100 * share:.3f} %)")
    assert share <= 0.01
