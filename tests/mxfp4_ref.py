"""CPU restatement of the MXFP4 weight format of llm_weight_dtype = "fp4" (include/unimedvl_hip.h, "MXFP4 weights").

    block = 32 consecutive k of one row;  e = the smallest integer with 6 * 2^e >= max|W[block]|, clamped to [-127, 127]
            (0 for an all-zero block), stored as the E8M0 byte e + 127;  s = 2^e
    q     = round-to-nearest-even e2m1(W / s), ties to the even code, the sign kept (a negative value that rounds to zero is
            code 8, -0)
    W'    = q * s                                                   (exact in bf16)

Everything is computed in float64 from the explicit e2m1 table, independently of the kernels' threshold form.  The model with
fp4 weights IS the bf16 model on W' for its seven linears per expert, lm_head on the e4m3 W' of oracle.fp8.
"""
import torch

from oracle.fp8 import LLM_LINEAR_SUFFIXES, quantize_rows

E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
CODE_VALUES = torch.tensor(list(E2M1) + [-v for v in E2M1], dtype=torch.float64)      # code 8 is -0.0
BLOCK = 32


def block_exponent(amax: torch.Tensor) -> torch.Tensor:
    """int64 e of every block maximum (float64 tensor): amax = m * 2^E with m in [0.5, 1), and 6 * 2^e >= m * 2^E  <=>
    2^(e - E) >= m / 6, whose smallest solution is e - E = -3 for m <= 0.75 and -2 above"""
    m, E = torch.frexp(amax)
    e = torch.where(m <= 0.75, E - 3, E - 2).to(torch.int64)
    return torch.where(amax > 0, e.clamp(-127, 127), torch.zeros_like(e))


def rne_e2m1(a: torch.Tensor) -> torch.Tensor:
    """magnitude code 0..7 of a >= 0 (float64) by round to nearest, ties to the even code"""
    mags = torch.tensor(E2M1, dtype=torch.float64)
    d = (a[..., None] - mags).abs()
    best = d.min(dim=-1, keepdim=True).values
    tied = d == best
    codes = torch.arange(8)
    # among the nearest codes take the even one (two nearest codes are always neighbours: one even, one odd)
    pick = torch.where(tied & (codes % 2 == 0), codes, torch.full_like(codes, 99)).min(dim=-1).values
    single = torch.where(tied, codes, torch.full_like(codes, 99)).min(dim=-1).values
    return torch.where(tied.sum(-1) > 1, pick, single)


def quantize(w: torch.Tensor):
    """w [N, K] (K % 32 == 0) -> (codes uint8 [N, K], e8m0 uint8 [N, K/32], W' bf16 [N, K])"""
    N, K = w.shape
    assert K % BLOCK == 0
    wf = w.detach().to(torch.float64).view(N, K // BLOCK, BLOCK)
    e = block_exponent(wf.abs().amax(dim=-1))
    s = torch.pow(torch.tensor(2.0, dtype=torch.float64), e.to(torch.float64))[..., None]
    mag = rne_e2m1(wf.abs() / s)
    codes = (mag + 8 * torch.signbit(wf).to(torch.int64)).to(torch.uint8)
    deq64 = CODE_VALUES[codes.long()] * s
    deq = deq64.to(torch.float32).to(torch.bfloat16)
    assert torch.equal(deq.to(torch.float64), deq64), "W' must be exact in bf16"
    return codes.view(N, K), (e + 127).to(torch.uint8), deq.view(N, K)


def image_bytes(N: int, K: int) -> int:
    np_, kt8 = ((N + 15) // 16 + 1) // 2, (K + 63) // 64
    return np_ * kt8 * (1024 + 64)


def unpack_image(img: torch.Tensor, N: int, K: int, swiglu_I: int = 0):
    """Invert the image of umv_quantize_pack_weight_mxfp4 -> (codes uint8 [rows, K], e8m0 uint8 [rows, K/32]); rows = N, or
    [2, I, ...] stacked gate / up when swiglu_I > 0 (N = 2 I)."""
    ntt, kt8 = (N + 15) // 16, (K + 63) // 64
    np_ = (ntt + 1) // 2
    b = img.cpu()
    assert b.numel() == image_bytes(N, K)
    c = b[:np_ * kt8 * 1024].view(np_, kt8, 4, 16, 2, 2, 4)             # [p][kt8][g][r][i][h][byte]
    nib = torch.stack([c & 0xF, c >> 4], dim=-1).reshape(np_, kt8, 4, 16, 2, 2, 8)   # element j = 2 * byte + (high nibble)
    codes = nib.permute(0, 4, 3, 1, 5, 2, 6).reshape(np_ * 32, kt8 * 64)[:, :K]      # row (2p+i)*16 + r, k = kt8*64 + h*32 + g*8 + j
    sc = b[np_ * kt8 * 1024:].view(np_, kt8, 16, 2, 2)                  # [p][kt8][r][i][h]
    scales = sc.permute(0, 3, 2, 1, 4).reshape(np_ * 32, kt8 * 2)[:, :K // BLOCK]
    if swiglu_I:
        def split(t):
            t = t[:ntt * 16].reshape(ntt // 2, 2, 16, t.shape[1])
            return torch.stack([t[:, 0].reshape(-1, t.shape[-1])[:swiglu_I], t[:, 1].reshape(-1, t.shape[-1])[:swiglu_I]])
        return split(codes), split(scales)
    return codes[:N], scales[:N]


def dequantised_weights_mxfp4(weights: dict) -> dict:
    """state dict -> the same dict with every LLM linear weight of both experts replaced by its MXFP4 W' and lm_head by its e4m3 W'"""
    out = {}
    for name, t in weights.items():
        base = name.rsplit(".", 1)[0]
        if not (name.endswith(".weight") and name.startswith("language_model.")):
            out[name] = t
        elif base.endswith("lm_head"):
            out[name] = quantize_rows(t)[2].to(t.dtype)
        elif any(base.endswith(s) or base.endswith(s + "_moe_gen") for s in LLM_LINEAR_SUFFIXES):
            out[name] = quantize(t)[2].to(t.dtype)
        else:
            out[name] = t
    return out
