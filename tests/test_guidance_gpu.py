"""umv_logit_guidance_bf16 and umv_guidance_feed (include/unimedvl_hip.h, "classifier-free guidance for text") at kernel level.

The combined logits are held bit for bit against the numpy model of the definition (tests/guidance_ref.py) evaluated with the lse[]
words the kernel itself wrote; those words against the fp64 log-sum-exp within the header's 1e-4 and - where the lm_head epilogue's
own statistics serve - bit for bit against the step ends' merge of them; the rewritten tiles against the shared tile recomputation run
over the model's row (the penalty kernel with neutral parameters, as tests/test_constraint_gpu.py does) and against the fp64 model
(maximum exact, sum within 1e-5 relative: 16 fast fp32 exponentials in a tree of four roundings).  Rows that are not active keep every
bit.  The logits live in a buffer framed by guard elements (tests/guarded.py)."""
import functools

import numpy as np
import pytest
import torch

import guidance_ref as G
import penalty_ref as P
from guarded import GUARD, Guarded

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
T = 0.7
SEED = 4321
K = 512
BOUND = 1e-4          # of a log-probability (include/unimedvl_hip.h, token log-probabilities)
SUM_RTOL = 1e-5       # of a tile's sum of exponentials against fp64
MODES = [(0.0, True), (0.0, False), (T, True), (T, False)]        # (temperature: 0 = greedy, with lse_partial)
NINF, NAN = 0xFF80, 0x7FC0


def _ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from unimedvl_amd import ops
    return ops


CH = __import__("unimedvl_amd.ops", fromlist=["CONSTRAIN_CHUNK"]).CONSTRAIN_CHUNK
VS = [40, 330, CH + 56]      # a partial last tile; 21 tiles; two chunks with a partial tile


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def _from_bits(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(BF16)


def _eq_stats(a, b):
    a, b = a.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32)
    fa, fb = a.view(np.float32), b.view(np.float32)
    return ((a == b) | (np.isnan(fa) & np.isnan(fb))).all()


@functools.lru_cache(maxsize=None)
def _problem(M, V):
    """x [M, K] and the packed lm_head weight [V, K] on the device: logits ~ N(0, 3^2)"""
    ops = _ops()
    g = torch.Generator().manual_seed(100 * M + V)
    x = torch.randn(M, K, generator=g).to(BF16).cuda()
    w = (torch.randn(V, K, generator=g) * (3.0 / K ** 0.5)).to(BF16).cuda()
    return x, ops.PackedLinear.from_weight(w)


def _lm_head(x, lin, temp, lse, step=None):
    """the lm_head call: (logits with a row stride beyond V, argmax_partial, lse_partial or None)"""
    ops = _ops()
    M, V = x.shape[0], lin.N
    nt = (V + 15) // 16
    out = torch.empty((M, (V + 7) // 8 * 8 + 8), dtype=BF16, device="cuda")[:, :V]
    keys = torch.zeros((M, nt), dtype=torch.int64, device="cuda")
    stats = torch.full((M, nt, 2), 55.0, dtype=torch.float32, device="cuda") if lse else None
    ops.gemm(x, lin, out=out, argmax_partial=keys, lse_partial=stats, sample=(temp, SEED, step) if temp > 0 else None)
    return out, keys, stats


def _all_tiles_through_penalty_tile(logits, temp, lse, step=None):
    """keys and statistics of EVERY tile of `logits` as the shared tile recomputation leaves them: the penalty kernel with neutral
    parameters, an id nothing records and a visit list that names one column of every tile"""
    ops = _ops()
    M, V = logits.shape
    nt = (V + 15) // 16
    keys = torch.zeros((M, nt), dtype=torch.int64, device="cuda")
    stats = torch.full((M, nt, 2), 55.0, dtype=torch.float32, device="cuda") if lse else None
    lst = (torch.arange(nt, dtype=torch.int32, device="cuda") * 16).repeat(M, 1).contiguous()
    before = logits.clone()
    ops.logit_penalty(logits, torch.full((M,), -1, dtype=torch.int64, device="cuda"), torch.zeros((M, V), dtype=torch.int32, device="cuda"),
                      lst, torch.full((M,), nt, dtype=torch.int32, device="cuda"), nt, temperature=temp, seed=SEED, step=step,
                      argmax_partial=keys, lse_partial=stats)
    assert torch.equal(before.view(torch.int16), logits.view(torch.int16)), "the neutral penalty call must leave the logits"
    return keys, stats


def _check_tiles_against_model(bits, keys, stats, temp, what):
    """one row: greedy keys exact, statistics against fp64 (maximum exact, sum within SUM_RTOL)"""
    if temp == 0:
        assert np.array_equal(keys.cpu().numpy().view(np.uint64), P.greedy_keys(bits)), f"{what}: greedy keys against the model"
    if stats is not None:
        m, s = P.tile_stats(bits, temp)
        got = stats.cpu().numpy().astype(np.float64)
        ok_m = (got[:, 0] == m) | (np.isnan(got[:, 0]) & np.isnan(m))
        ok_s = (np.abs(got[:, 1] - s) <= SUM_RTOL * np.abs(s)) | (np.isnan(got[:, 1]) & np.isnan(s))
        assert ok_m.all() and ok_s.all(), f"{what}: statistics against the fp64 model, tiles {np.flatnonzero(~(ok_m & ok_s))[:6]}"


class Framed:
    """[M, V] bf16 logits with row stride V + pad inside a guarded buffer (the pad columns hold the guard pattern too)"""

    def __init__(self, bits, pad):
        M, V = bits.shape
        self.M, self.V, self.ld = M, V, V + pad
        self.g = Guarded(M * self.ld, BF16)
        self.all = self.g.raw[GUARD:GUARD + M * self.ld].view(BF16).view(M, self.ld)
        self.logits = self.all[:, :V]
        self.logits.copy_(_from_bits(bits).cuda())

    def fetch(self):
        """the rows' bits, after checking the guards and the pad columns"""
        typed, raw = self.g.fetch()
        raw = raw.view(self.M, self.ld)
        assert bool((raw[:, self.V:] == self.g.pat).all()), "the columns behind V were written"
        return raw[:, :self.V].contiguous().numpy().view(np.uint16)


def _words(M):
    """guarded fp32 [M] outputs: (Guarded, the tensor view)"""
    g = Guarded(M, torch.float32)
    return g, g.raw[GUARD:GUARD + M].view(torch.float32)


def _pad(V, aligned):
    return (-V) % 8 + 8 if aligned else (-V) % 8 + 3


# ----------------------------------------------------------------------------- the tables of the cases
def _tables(R):
    """(pair, scale, beta) per row.  2: one pair; 6: two pairs whose unconditional rows are not adjacent to them, two free rows;
    64: 32 pairs over every scale of the definition, g == 1 included, and three bad pair words"""
    if R == 2:
        return [1, -1], [3.0, 1.0], [0.0, 0.0]
    if R == 6:
        return [3, -1, 5, -1, -1, -1], [1.5, 1.0, 0.5, 1.0, 1.0, 1.0], [0.0, 0.0, 0.1, 0.0, 0.0, 0.0]
    pair = [c + 32 for c in range(32)] + [-1] * 32
    pair[5], pair[6], pair[7] = 64, 6, -7                     # outside, itself, negative: rows 5 - 7 (and 37 - 39) take no part
    scale = [(0.0, 0.5, 1.0, 1.5, 3.0)[c % 5] for c in range(32)] + [1.0] * 32
    beta = [(0.0, 0.0, 0.0, 0.1, 0.9, 0.0, 0.0)[c % 7] for c in range(32)] + [0.0] * 32
    return pair, scale, beta


def _dev_tables(pair, scale, beta):
    lb = np.array([G.log_beta(b) for b in beta], dtype=np.float32)
    return (torch.tensor(pair, dtype=torch.int32, device="cuda"), torch.tensor(scale, dtype=torch.float32, device="cuda"),
            torch.from_numpy(lb).cuda(), lb)


def _guide(fr, pair, scale, beta, temp, keys, stats, step, use_stats=None):
    """the stage on a Framed buffer: (rows' bits after, lse words, row_max words, the guards of the two)"""
    ops = _ops()
    tp, ts, tb, lb = _dev_tables(pair, scale, beta)
    M, nt = fr.M, (fr.V + 15) // 16
    gl, lse = _words(M)
    gm, mx = _words(M)
    reuse = stats is not None and temp in (0.0, 1.0)
    scratch = None if (reuse if use_stats is None else not use_stats) else torch.full((M, nt, 2), 66.0, dtype=torch.float32, device="cuda")
    ops.logit_guidance(fr.logits, tp, ts, tb, lse, mx, stats=scratch, temperature=temp, seed=SEED, step=step, argmax_partial=keys,
                       lse_partial=stats)
    return fr.fetch(), gl.fetch()[0].numpy().copy(), gm.fetch()[0].numpy().copy(), gl, lb


def _model(raw, pair, scale, lb, lse):
    """the model's rows with the kernel's own lse words; (rows, the active rows)"""
    out, active = raw.copy(), []
    for c in range(len(pair)):
        u = G.partner(pair, scale, c)
        if u >= 0:
            out[c] = G.combine_row(raw[c], raw[u], lse[c], lse[u], scale[c], lb[c])
            if G.row_max(raw[c]) != -np.inf:
                active.append(c)
    return out, active


def _check_lse(raw, pair, scale, lse, mx, gl, what):
    part = G.takes_part(pair, scale)
    pat = np.array([gl.pat], dtype=np.int32).view(np.float32)[0]
    worst = 0.0
    for r, p in enumerate(part):
        if not p:
            assert lse[r:r + 1].view(np.int32)[0] == gl.pat and np.isnan(pat), f"{what}: lse[{r}] of a row that takes no part was written"
            continue
        want = G.lse64(raw[r])
        assert mx[r] == G.row_max(raw[r]), f"{what}: row_max[{r}]"
        if np.isnan(want) or np.isinf(want):
            assert (np.isnan(want) and np.isnan(lse[r])) or want == lse[r], f"{what}: lse[{r}] = {lse[r]}, fp64 {want}"
        else:
            worst = max(worst, abs(float(lse[r]) - want))
    print(f"{what}: lse off the fp64 value by at most {worst:.3g}")
    assert worst <= BOUND, what


# ----------------------------------------------------------------------------- 1. against the lm_head epilogue and the model
@pytest.mark.parametrize("R", [2, 6, 64])
@pytest.mark.parametrize("V", VS)
def test_guided_rows_against_the_epilogue_and_the_model(V, R):
    ops = _ops()
    pair, scale, beta = _tables(R)
    x, lin = _problem(R, V)
    step = torch.tensor([3], dtype=torch.int64, device="cuda")
    for temp, lse_on in MODES:
        out, keys, stats = _lm_head(x, lin, temp, lse_on, step)
        raw = _bits(out)
        fr = Framed(raw, _pad(V, True))
        before = (keys.clone(), stats.clone() if lse_on else None)
        merged = None
        if temp == 0 and lse_on:       # the step ends' merge of the epilogue's own statistics: -logf(S) (the target is the maximum)
            rm = torch.from_numpy(np.array([G.row_max(r) for r in raw], dtype=np.float32)).cuda()
            neg_log_s = ops.token_logprob_from_stats(stats, rm, torch.zeros(R, dtype=torch.int64, device="cuda"), V).cpu().numpy()
            merged = rm.cpu().numpy() + (-neg_log_s)
        act = [c for c in range(R) if G.partner(pair, scale, c) >= 0]
        at = torch.tensor(act, device="cuda")
        keys[at] = 0                                   # poison what the kernel must write: every tile of an active row
        if lse_on and temp != 0:
            stats[at] = 55.0
        got, lse, mx, gl, lb = _guide(fr, pair, scale, beta, temp, keys, stats, step)
        tag = f"V={V} R={R} T={temp} lse={lse_on}"
        _check_lse(raw, pair, scale, lse, mx, gl, tag)
        if merged is not None:
            part = np.array(G.takes_part(pair, scale))
            assert np.array_equal(lse[part].view(np.uint32), merged.astype(np.float32)[part].view(np.uint32)), \
                f"{tag}: lse[] is not the merge of the epilogue's own lse_partial"
        model, active = _model(raw, pair, scale, lb, lse)
        assert sorted(active) == act and P.same_bits(got, model).all(), f"{tag}: combined logits, rows {np.flatnonzero((got != model).any(1))[:6]}"
        assert all((got[c] != raw[c]).any() for c in act), f"{tag}: an active row did not move"
        tk, ts = _all_tiles_through_penalty_tile(_from_bits(got).cuda(), temp, lse_on, step)       # (got is the model's row, bit for bit)
        for m in range(R):
            if m not in act:                           # free rows, unconditional rows, g == 1 rows, bad pair words: every bit stays
                assert np.array_equal(got[m], raw[m]), f"{tag} row {m}: logits of an untouched row"
                assert torch.equal(keys[m], before[0][m]), f"{tag} row {m}: keys of an untouched row"
                assert not lse_on or _eq_stats(stats[m], before[1][m]), f"{tag} row {m}: statistics of an untouched row"
                continue
            assert torch.equal(keys[m], tk[m]), f"{tag} row {m}: keys differ from the shared tile recomputation's"
            assert not lse_on or _eq_stats(stats[m], ts[m]), f"{tag} row {m}: statistics differ from the shared tile recomputation's"
            _check_tiles_against_model(model[m], keys[m], stats[m] if lse_on else None, temp, f"{tag} row {m}")


# ----------------------------------------------------------------------------- 2. crafted rows, aligned and unaligned row strides
def _crafted(V):
    """(name, conditional bits, unconditional bits, g, beta)"""
    rng = np.random.default_rng(V + 1)

    def rnd():
        return P.bf16_bits((rng.standard_normal(V) * 3).astype(np.float32))
    one = P.bf16_bits(np.array([2.5], dtype=np.float32))[0]
    cases = [("random", rnd(), rnd(), 3.0, 0.0), ("g = 0", rnd(), rnd(), 0.0, 0.0), ("g = 0.5", rnd(), rnd(), 0.5, 0.0),
             ("floor 0.1", rnd(), rnd(), 3.0, 0.1), ("floor 0.9", rnd(), rnd(), 1.5, 0.9)]
    c, u = rnd(), rnd()
    c[[0, 5, V - 1]] = NINF
    cases.append(("-inf in the conditional row", c, u, 3.0, 0.0))
    c, u = rnd(), rnd()
    u[[1, 17 % V, V - 2]] = NINF
    c[1] = NINF                                                   # both: banned stays banned
    cases.append(("-inf in the unconditional row", c, u, 3.0, 0.0))
    c, u = rnd(), rnd()
    c[3] = NAN
    cases.append(("NaN in the conditional row", c, u, 1.5, 0.0))
    c, u = rnd(), rnd()
    u[V - 1], u[4] = NAN, 0xFFC1
    cases.append(("NaN in the unconditional row", c, u, 1.5, 0.0))
    cases.append(("conditional row of -inf only", np.full(V, NINF, dtype=np.uint16), rnd(), 3.0, 0.0))
    cases.append(("unconditional row of -inf only", rnd(), np.full(V, NINF, dtype=np.uint16), 3.0, 0.0))
    c, u = rnd(), rnd()
    c[rng.choice(V, V // 3, replace=False)] = one                 # ties at the top of the conditional row ...
    u[:] = one                                                    # ... against a flat unconditional row
    c[np.argmax(P.bf16_float(c))] = one
    cases.append(("ties", c, u, 3.0, 0.9))
    c = rnd()
    cases.append(("the same row twice", c, c.copy(), 3.0, 0.0))
    cases.append(("g = 1", rnd(), rnd(), 1.0, 0.0))
    return cases


@pytest.mark.parametrize("aligned", [True, False])          # 16-byte aligned rows, or the scalar path
@pytest.mark.parametrize("V", VS)
def test_crafted_rows(V, aligned):
    cases = _crafted(V)
    n = len(cases)
    M = 2 * n
    raw = np.stack([c[1] for c in cases] + [c[2] for c in cases])       # conditional rows first, their partners behind
    pair = list(range(n, M)) + [-1] * n
    scale = [c[3] for c in cases] + [1.0] * n
    beta = [c[4] for c in cases] + [0.0] * n
    step = torch.tensor([5], dtype=torch.int64, device="cuda")
    for temp, lse_on in MODES:
        fr = Framed(raw, _pad(V, aligned))
        keys, stats = _all_tiles_through_penalty_tile(_from_bits(raw).cuda(), temp, lse_on, step)     # what the epilogue leaves
        before = (keys.clone(), stats.clone() if lse_on else None)
        got, lse, mx, gl, lb = _guide(fr, pair, scale, beta, temp, keys, stats, step)
        tag = f"V={V} aligned={aligned} T={temp} lse={lse_on}"
        _check_lse(raw, pair, scale, lse, mx, gl, tag)
        model, active = _model(raw, pair, scale, lb, lse)
        bad = [cases[m % n][0] for m in range(M) if not P.same_bits(got[m], model[m]).all()]
        assert not bad, f"{tag}: rows {bad}"
        # (over the row as stored: the model's row bit for bit, but for the payload of a NaN, which the keys order by)
        tk, ts = _all_tiles_through_penalty_tile(_from_bits(got).cuda(), temp, lse_on, step)
        names = [c[0] for c in cases]
        assert names.index("conditional row of -inf only") not in active and names.index("g = 1") not in active
        for m in range(M):
            name = cases[m % n][0]
            if m not in active:
                assert np.array_equal(got[m], raw[m]) and torch.equal(keys[m], before[0][m]) and \
                    (not lse_on or _eq_stats(stats[m], before[1][m])), f"{tag} {name}: an untouched row was written"
                continue
            assert torch.equal(keys[m], tk[m]), f"{tag} {name}: keys"
            assert not lse_on or _eq_stats(stats[m], ts[m]), f"{tag} {name}: statistics"
            if not np.isnan(P.bf16_float(got[m])).all():      # (the fp64 model has no maximum for a tile of NaN only; the kernels' is -inf)
                _check_tiles_against_model(got[m], keys[m], stats[m] if lse_on else None, temp, f"{tag} {name}")
        # what the cases are there for
        f = P.bf16_float(got)
        i = names.index("-inf in the conditional row")
        assert (got[i][[0, 5, V - 1]] == NINF).all()
        i = names.index("-inf in the unconditional row")
        assert got[i][1] == NINF and np.isfinite(f[i][[17 % V, V - 2]]).all()
        assert np.isnan(f[names.index("NaN in the conditional row")]).any() and np.isnan(f[names.index("NaN in the unconditional row")][V - 1])
        for i, b in ((names.index("floor 0.1"), 0.1), (names.index("floor 0.9"), 0.9), (names.index("ties"), 0.9)):
            keep = G.kept_by_floor(raw[i], b)
            assert np.array_equal(got[i] != NINF, keep) and keep[np.argmax(P.bf16_float(raw[i]))], f"{tag}: the floor at beta = {b}"
    # the logits only: no partials
    fr = Framed(raw, _pad(V, aligned))
    got, lse, mx, gl, lb = _guide(fr, pair, scale, beta, 0.0, None, None, None)
    assert P.same_bits(got, _model(raw, pair, scale, lb, lse)[0]).all()


# ----------------------------------------------------------------------------- 3. picks against the independent entries
def _step_bufs(B, max_len, s):
    dev = "cuda"
    return dict(slot=torch.zeros(B, dtype=torch.int32, device=dev), pos=torch.zeros(B, dtype=torch.int32, device=dev),
                kvl=torch.ones(B, dtype=torch.int32, device=dev), ids=torch.full((B,), -5, dtype=torch.int64, device=dev),
                in_ids=torch.zeros((max_len, B), dtype=torch.int64, device=dev), pred=torch.zeros((max_len, B), dtype=torch.int64, device=dev),
                step=torch.full((B,), s, dtype=torch.int64, device=dev), lp=torch.zeros((max_len, B), dtype=torch.float32, device=dev),
                cut=torch.zeros((max_len, B), dtype=torch.float32, device=dev), kept=torch.zeros((max_len, B), dtype=torch.int32, device=dev))


def _guided(R, V, temp, lse_on, s=2):
    """lm_head call, then the stage: (guided logits, keys, stats, step buffers)"""
    pair, scale, beta = _tables(R)
    x, lin = _problem(R, V)
    b = _step_bufs(R, 4, s)
    out, keys, stats = _lm_head(x, lin, temp, lse_on, b["step"])
    fr = Framed(_bits(out), _pad(V, True))
    _guide(fr, pair, scale, beta, temp, keys, stats, b["step"])
    return fr.logits, keys, stats, b


def _check_logprobs(lp, alone, logits, ids, temp, what):
    bits = _bits(logits)
    worst = 0.0
    for m in range(bits.shape[0]):
        worst = max(worst, abs(float(lp[m]) - float(alone[m])), abs(float(lp[m]) - P.logprob(bits[m], int(ids[m]), temp)))
    print(f"{what}: log-probability off the stand-alone entry / the fp64 log-softmax of the combined row by at most {worst:.3g}")
    assert worst <= BOUND, what


@pytest.mark.parametrize("R", [6, 64])
@pytest.mark.parametrize("V", VS)
def test_fused_picks_equal_the_stand_alone_entries_on_the_combined_logits(V, R):
    ops = _ops()
    s = 2
    out, keys, _, b = _guided(R, V, 0.0, False, s)
    ops.decode_step_end_argmax(b["slot"], b["pos"], b["kvl"], keys, b["ids"], b["in_ids"], b["pred"], b["step"])
    assert torch.equal(b["ids"], ops.argmax(out)), "greedy"
    out, keys, stats, b = _guided(R, V, 0.0, True, s)
    ops.decode_step_end_logprob(b["slot"], b["pos"], b["kvl"], keys, stats, b["ids"], b["in_ids"], b["pred"], b["step"], out, b["lp"], 0.0)
    assert torch.equal(b["ids"], ops.argmax(out)), "greedy with log-probabilities"
    _check_logprobs(b["lp"][s].cpu(), ops.token_logprob(out, b["ids"], 0.0).cpu(), out, b["ids"], 0.0, f"V={V} R={R} greedy")
    out, keys, _, b = _guided(R, V, T, False, s)
    st = b["step"][:1].clone()
    ops.decode_step_end_argmax(b["slot"], b["pos"], b["kvl"], keys, b["ids"], b["in_ids"], b["pred"], b["step"])
    assert torch.equal(b["ids"], ops.sample(out, T, SEED, step=st)), "sampling"
    out, keys, stats, b = _guided(R, V, T, True, s)
    flt = dict(top_k=5, top_p=0.8)
    cut = torch.zeros(R, dtype=torch.float32, device="cuda")
    kept = torch.zeros(R, dtype=torch.int32, device="cuda")
    alone = ops.sample_truncated(out, T, SEED, step=b["step"][:1].clone(), cut_y=cut, n_kept=kept, **flt)
    ops.decode_step_end_truncated(b["slot"], b["pos"], b["kvl"], keys, b["ids"], b["in_ids"], b["pred"], b["step"], out, T, SEED,
                                  lse_partial=stats, logprobs=b["lp"], cut_y=b["cut"], n_kept=b["kept"], **flt)
    assert torch.equal(b["ids"], alone), "truncated: ids"
    assert torch.equal(b["cut"][s].view(torch.int32), cut.view(torch.int32)) and torch.equal(b["kept"][s], kept), "truncated: cutoff"
    _check_logprobs(b["lp"][s].cpu(), ops.token_logprob(out, b["ids"], T).cpu(), out, b["ids"], T, f"V={V} R={R} truncated")


# ----------------------------------------------------------------------------- 4. batch independence
@pytest.mark.parametrize("V", [330, VS[2]])
def test_a_pair_does_not_depend_on_its_batch(V):
    """the pair (2, 5) of the six-row batch alone as rows (0, 1): the same logits and lse words - and, greedy, the same keys and
    statistics (the scalar sampling key names the row index, so sampled keys are not comparable across rows)"""
    pair, scale, beta = _tables(6)
    x, lin = _problem(6, V)
    step = torch.tensor([1], dtype=torch.int64, device="cuda")
    for temp in (0.0, T):
        out, keys, stats = _lm_head(x, lin, temp, True, step)
        fr = Framed(_bits(out), _pad(V, True))
        got, lse, _, _, _ = _guide(fr, pair, scale, beta, temp, keys, stats, step)
        o2, k2, s2 = _lm_head(x[[2, 5]].contiguous(), lin, temp, True, step)
        assert np.array_equal(_bits(o2), _bits(out)[[2, 5]]), "the lm_head rows themselves"
        f2 = Framed(_bits(o2), _pad(V, True))
        got2, lse2, _, _, _ = _guide(f2, [1, -1], [scale[2], 1.0], [beta[2], 0.0], temp, k2, s2, step)
        assert np.array_equal(got2, got[[2, 5]]) and np.array_equal(lse2.view(np.uint32), lse[[2, 5]].view(np.uint32)), f"T={temp}"
        if temp == 0:
            assert torch.equal(k2[0], keys[2]) and _eq_stats(s2[0], stats[2])


# ----------------------------------------------------------------------------- 5. the feed
@pytest.mark.parametrize("R", [2, 6, 64])
def test_feed_writes_exactly_the_partner_words(R):
    ops = _ops()
    pair, scale, _ = _tables(R)
    tp = torch.tensor(pair, dtype=torch.int32, device="cuda")
    max_len = 4
    g = torch.Generator().manual_seed(R)
    for s_next in (0, 1, 3, 4, 9):                       # the step counter as the step end left it: s = s_next - 1 is the step just ended
        ids = torch.randint(0, 1000, (R + 2,), generator=g).cuda()
        in_ids = torch.randint(0, 1000, (max_len + 2, R), generator=g).cuda()
        pred = torch.randint(0, 1000, (max_len + 2, R), generator=g).cuda()
        step = torch.full((R,), s_next, dtype=torch.int64, device="cuda")
        want = (ids.clone(), in_ids.clone(), pred.clone())
        for c in range(R):
            u = G.partner(pair, scale, c, use_scale=False)      # (a pair at scale 1 is fed too)
            if u < 0:
                continue
            want[0][1 + u] = want[0][1 + c]
            s = s_next - 1
            if 0 <= s < max_len:
                want[2][1 + s, u] = want[2][1 + s, c]
            if 0 <= s + 1 < max_len:
                want[1][1 + s + 1, u] = want[1][1 + s + 1, c]
        ops.guidance_feed(tp, ids[1:R + 1], in_ids[1:max_len + 1], pred[1:max_len + 1], step)
        assert torch.equal(ids, want[0]) and torch.equal(in_ids, want[1]) and torch.equal(pred, want[2]), f"R={R} step {s_next}"
        assert torch.equal(step, torch.full((R,), s_next, dtype=torch.int64, device="cuda"))
    assert any(G.partner(pair, scale, c, use_scale=False) >= 0 for c in range(R))


# ----------------------------------------------------------------------------- 6. arguments
def test_argument_errors_launch_nothing():
    ops = _ops()
    from unimedvl_amd._lib import UmvError
    V = 40
    bits = P.bf16_bits(np.linspace(-3, 3, 2 * V).astype(np.float32)).reshape(2, V)
    logits = _from_bits(bits).cuda()
    tp, ts, tb, _ = _dev_tables([1, -1], [3.0, 1.0], [0.0, 0.0])
    lse, mx = torch.zeros(2, device="cuda"), torch.zeros(2, device="cuda")
    keys = torch.zeros((2, 3), dtype=torch.int64, device="cuda")
    stats = torch.zeros((2, 3, 2), dtype=torch.float32, device="cuda")
    scratch = torch.zeros((2, 3, 2), dtype=torch.float32, device="cuda")
    ok = dict(stats=scratch)
    for kw in (dict(ok, temperature=-0.5), dict(ok, temperature=float("nan")), dict(ok, temperature=float("inf")),
               dict(ok, lse_partial=stats),                                                           # goes with argmax_partial
               dict(ok, argmax_partial=torch.zeros((2, 4), dtype=torch.int64, device="cuda")),        # not the tile count of V
               dict(),                                                                                # no statistics and no workspace
               dict(argmax_partial=keys, lse_partial=stats, temperature=0.7),                         # ... none that serves at T = 0.7
               dict(stats=torch.zeros((2, 4, 2), dtype=torch.float32, device="cuda"))):
        with pytest.raises(UmvError):
            ops.logit_guidance(logits, tp, ts, tb, lse, mx, **kw)
    for args in ((tp[:1], ts, tb, lse, mx), (tp.to(torch.int64), ts, tb, lse, mx), (tp, ts[:1], tb, lse, mx), (tp, ts, tb.double(), lse, mx),
                 (tp, ts, tb, lse[:1], mx), (tp, None, tb, lse, mx), (tp, ts, tb, lse, None), (tp.cpu(), ts, tb, lse, mx)):
        with pytest.raises(UmvError):
            ops.logit_guidance(logits, *args, stats=scratch)
    with pytest.raises(UmvError):
        ops.logit_guidance(logits.float(), tp, ts, tb, lse, mx, stats=scratch)
    ids = torch.zeros(2, dtype=torch.int64, device="cuda")
    hist = torch.zeros((4, 2), dtype=torch.int64, device="cuda")
    step = torch.ones(2, dtype=torch.int64, device="cuda")
    for args in ((tp, ids[:1], hist, hist, step), (tp, ids, hist[:, :1], hist, step), (tp, ids, hist, hist[:2], step),
                 (tp, ids.to(torch.int32), hist, hist, step), (tp.to(torch.int64), ids, hist, hist, step), (tp, ids, hist, hist, step[:1])):
        with pytest.raises(UmvError):
            ops.guidance_feed(*args)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(logits), bits) and not lse.any() and not mx.any() and not keys.any() and not ids.any() and not hist.any(), \
        "a refused call wrote something"
    ops.logit_guidance(logits, tp, ts, tb, lse, mx, argmax_partial=keys, lse_partial=stats, stats=scratch, temperature=0.7)
    ops.guidance_feed(tp, ids, hist, hist.clone(), step)
