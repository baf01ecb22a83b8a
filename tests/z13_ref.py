"""CPU restatement (numpy) of the exact 13-bit weight image "z13" (include/unimedvl_hip.h, "exact 13-bit image of bf16 weights").

    unit    = a pair of 16-row n-tiles (2p, 2p + 1) x 64 k; lane = ((k % 32) / 8) * 16 + n % 16 holds the 32 weights of the bf16
              image's fragments (tile 2p + tt, k half h, j = k % 8), fragment number f = 2 tt + h
    base[p] = the largest exponent field below 255 among the pair's rows that exist (0 when there is none)
    code    = base - field, codable when field != 255 and 0 <= code <= 30; an uncodable weight is written as code 0 and, in a row
              that exists, flags its (pair, 512-k block)
    bits    = s << 15 | (base - code) << 7 | m7

Everything works on uint16 bit patterns; nothing here shares code with the kernels.
"""
import numpy as np

RECORD = 3328


def head_bytes(NP):
    return (NP * 16 + 255) // 256 * 256


def image_bytes(N, K):
    ntt = (N + 15) // 16
    NP = (ntt + 1) // 2
    return head_bytes(NP) + NP * (K // 64) * RECORD


def bf16_image(w):
    """[N, K] uint16 bit patterns (K % 32 == 0) -> the packed bf16 image [ceil(N/16), K/32, 64 lanes, 8], zero padded"""
    N, K = w.shape
    ntt = (N + 15) // 16
    p = np.zeros((ntt * 16, K), np.uint16)
    p[:N] = w
    # [nt, r, kt, g, j] -> [nt, kt, g, r, j]
    return np.ascontiguousarray(p.reshape(ntt, 16, K // 32, 4, 8).transpose(0, 2, 3, 1, 4)).reshape(ntt, K // 32, 64, 8)


def bf16_image_swiglu(gate, up):
    """gate / up [I, K] (I % 16 == 0) -> the packed image of the [2I, K] SwiGLU weight: 16-row tiles interleaved"""
    g, u = bf16_image(gate), bf16_image(up)
    return np.stack([g, u], axis=1).reshape(2 * g.shape[0], *g.shape[1:])


def _pairs(img16, N):
    """image [NTT, KT, 64, 8] -> w [NP, tt, u, h, lane, j], exists [NP, tt, 1, 1, lane, 1] (row below N), tile_there [NP, tt]"""
    ntt, KT = img16.shape[:2]
    assert KT % 2 == 0
    NP = (ntt + 1) // 2
    full = np.zeros((2 * NP, KT, 64, 8), np.uint16)
    full[:ntt] = img16
    w = full.reshape(NP, 2, KT // 2, 2, 64, 8)
    tile = np.arange(2 * NP).reshape(NP, 2)
    rows = tile[:, :, None] * 16 + (np.arange(64) % 16)[None, None, :]
    exists = (rows < N)[:, :, None, None, :, None]
    return w, exists, tile < ntt


def _byte_of(j):
    return 2 * (j & 1) + ((j >> 1) & 1)


def pack(img16, N):
    """-> (flags uint64 [NP], bases uint8 [NP], records uint8 [NP, KT8, 3328], flagged bool [NP, ceil(KT8/8)])"""
    w, exists, there = _pairs(img16, N)
    NP, _, KT8 = w.shape[:3]
    field = ((w >> 7) & 0xFF).astype(np.int64)
    counted = np.where(exists & (field != 255), field, 0)
    bases = counted.max(axis=(1, 2, 3, 4, 5))
    diff = bases[:, None, None, None, None, None] - field
    codable = (field != 255) & (diff >= 0) & (diff <= 30)
    code = np.where(codable, diff, 0)
    code = np.where(there[:, :, None, None, None, None], code, 0)        # the missing tile of a ragged last pair: zeros
    bad = (exists & ~codable).any(axis=(1, 3, 4, 5))                    # [NP, KT8]
    nblk = (KT8 + 7) // 8
    flagged = np.zeros((NP, nblk), bool)
    for u in range(KT8):
        flagged[:, u >> 3] |= bad[:, u]
    flags = np.zeros(NP, np.uint64)
    for b in range(nblk):
        flags |= flagged[:, b].astype(np.uint64) << np.uint64(b)
    rec = np.zeros((NP, KT8, RECORD), np.uint8)
    smb = (((w >> 8) & 0x80) | (w & 0x7F)).astype(np.uint8)             # [NP, tt, u, h, lane, j]
    # plane tt at tt*1024: lane*16 + 8h + j
    rec[:, :, :2048] = smb.transpose(0, 2, 1, 4, 3, 5).reshape(NP, KT8, 2048)
    nib = np.zeros((NP, 2, KT8, 2, 64), np.uint64)
    top = np.zeros((NP, KT8, 64), np.uint64)
    for j in range(8):
        B, q = _byte_of(j), j >> 2
        nib |= (code[..., j] & 15).astype(np.uint64) << np.uint64(8 * B + 4 * q)
        for tt in range(2):
            for h in range(2):
                f = 2 * tt + h
                top |= (code[:, tt, :, h, :, j] >> 4).astype(np.uint64) << np.uint64(8 * B + 2 * f + q)
    nibd = nib.astype(np.uint32).transpose(0, 2, 4, 1, 3).reshape(NP, KT8, 64, 4)       # [p, u, lane, f]
    rec[:, :, 2048:3072] = np.ascontiguousarray(nibd).view(np.uint8).reshape(NP, KT8, 1024)
    rec[:, :, 3072:] = np.ascontiguousarray(top.astype(np.uint32)).view(np.uint8).reshape(NP, KT8, 256)
    return flags, bases.astype(np.uint8), rec, flagged


def to_bytes(flags, bases, rec):
    NP = flags.shape[0]
    out = np.zeros(head_bytes(NP) + rec.size, np.uint8)
    head = out[:16 * NP].reshape(NP, 16)                    # per pair: flags u64, base u8, 7 zero bytes
    head[:, :8] = flags.view(np.uint8).reshape(NP, 8)
    head[:, 8] = bases
    out[head_bytes(NP):] = rec.reshape(-1)
    return out


def split_bytes(img, N, K):
    """the image's bytes -> (flags, bases, records)"""
    ntt = (N + 15) // 16
    NP, KT8 = (ntt + 1) // 2, K // 64
    img = np.asarray(img, np.uint8)
    assert img.size == image_bytes(N, K)
    head = img[:16 * NP].reshape(NP, 16)
    assert not head[:, 9:].any()
    flags = np.ascontiguousarray(head[:, :8]).view(np.uint64).reshape(NP)
    bases = head[:, 8].copy()
    rec = img[head_bytes(NP):].reshape(NP, KT8, RECORD)
    return flags, bases, rec


def unpack(bases, rec, ntt):
    """-> the bf16 image [ntt, KT, 64, 8] that the records decode to (whatever a flagged block holds included)"""
    NP, KT8 = rec.shape[:2]
    smb = rec[:, :, :2048].reshape(NP, KT8, 2, 64, 2, 8).transpose(0, 2, 1, 4, 3, 5).astype(np.int64)   # [p, tt, u, h, lane, j]
    nibd = np.ascontiguousarray(rec[:, :, 2048:3072]).view(np.uint32).reshape(NP, KT8, 64, 2, 2).transpose(0, 3, 1, 4, 2).astype(np.int64)
    top = np.ascontiguousarray(rec[:, :, 3072:]).view(np.uint32).reshape(NP, KT8, 64).astype(np.int64)
    code = np.zeros((NP, 2, KT8, 2, 64, 8), np.int64)
    for j in range(8):
        B, q = _byte_of(j), j >> 2
        code[..., j] = (nibd >> (8 * B + 4 * q)) & 15
        for tt in range(2):
            for h in range(2):
                code[:, tt, :, h, :, j] |= ((top >> (8 * B + 2 * (2 * tt + h) + q)) & 1) << 4
    E = (bases.astype(np.int64)[:, None, None, None, None, None] - code) & 0xFF
    bits = ((smb & 0x80) << 8) | (E << 7) | (smb & 0x7F)
    return bits.astype(np.uint16).reshape(2 * NP, KT8 * 2, 64, 8)[:ntt]


def block_mask(flagged, ntt, KT):
    """flagged [NP, blocks] -> bool [ntt, KT, 1, 1]: the image positions inside flagged blocks"""
    m = np.repeat(np.repeat(flagged, 2, axis=0), 16, axis=1)[:ntt, :KT]
    return m[:, :, None, None]
