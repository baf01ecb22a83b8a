"""fp64 restatement of the token log-probability (include/unimedvl_hip.h, "token log-probabilities") for the tests.

    y[n]     = float(bf16 logit[n])                      greedy (temperature 0)
             = bf16_round(fp32(logit[n]) / fp32(T))      sampling at temperature T > 0 (the reference's bf16 tensor logits / T)
    logprob  = y[id] - logsumexp_n y[n]                  a -inf column adds 0, a NaN column makes the row NaN
    (m_t, s_t) of a 16-column tile t = (max y, sum exp(y - m_t)) over its columns; a tile of -inf only is (-inf, 0)

Inputs are bf16 tensors (any device); everything after y is float64 on the CPU.  Nothing here shares code with the kernels.
"""
import torch

TILE = 16


def y_values(logits, temperature=0.0):
    """[M, V] bf16 -> [M, V] float64: the value the token pick orders, without noise"""
    assert logits.dtype == torch.bfloat16
    x = logits.detach().cpu()
    if temperature and temperature > 0:
        x = (x.float() / torch.tensor(temperature, dtype=torch.float32)).to(torch.bfloat16)
    return x.double()


def logsumexp(y):
    """[M, V] float64 -> [M]; rows of -inf only give -inf, rows with a NaN give NaN"""
    m = y.max(dim=-1).values
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    out = m + torch.log(torch.exp(y - m[:, None]).sum(-1))
    return torch.where(torch.isnan(y).any(-1), torch.full_like(out, float("nan")), out)


def logprob(logits, ids, temperature=0.0):
    """[M, V] bf16 logits, [M] ids -> [M] float64"""
    y = y_values(logits, temperature)
    ids = torch.as_tensor(ids, dtype=torch.int64).cpu().reshape(-1)
    return y.gather(1, ids[:, None])[:, 0] - logsumexp(y)


def tile_stats(logits, temperature=0.0):
    """[M, V] bf16 -> (m [M, ceil(V / 16)], s the same shape), float64"""
    y = y_values(logits, temperature)
    M, V = y.shape
    nt = (V + TILE - 1) // TILE
    pad = torch.full((M, nt * TILE), float("-inf"), dtype=torch.float64)
    pad[:, :V] = y
    t = pad.reshape(M, nt, TILE)
    m = t.max(-1).values
    ref = torch.where(torch.isinf(m) & (m < 0), torch.zeros_like(m), m)
    s = torch.exp(t - ref[..., None]).sum(-1)
    return m, s
