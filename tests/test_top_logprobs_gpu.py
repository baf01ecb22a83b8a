"""Top-n alternative tokens with log-probabilities, and token ranks (include/unimedvl_hip.h, "top-n alternative tokens and token
ranks") on the GPU, against the fp64 definition of tests/top_logprobs_ref.py on the very logits the call stored.

ids and ranks are exact.  The log-probabilities are the token log-probabilities' values (the same y, the same merged statistics, the
same finish), so their bound is that file's BOUND = 1e-4 absolute; every test prints the largest error it saw before it asserts.

Largest errors seen on an MI355X (`pytest -s`): 6.7e-7 on the GEMM's logits (V = 40 .. 4112, all three lm_head images), 9.5e-7 on the
crafted rows, 5.5e-7 in the sessions.
"""
import functools
import math

import numpy as np
import pytest
import torch

import top_logprobs_ref as R
from conftest import NEW_TOKEN_IDS
from test_logprob_gpu import BOUND, SEED, _case, _ctx, _finish, _gemm, _kv, _lin, _ops, _requests, _same, _session, _step_bufs, _x
from test_logprob_gpu import model  # noqa: F401  (the tiny engine fixture)

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
UNSET_I, UNSET_F = -77, 55.0


def _outs(max_len, B, n):
    return dict(ids=torch.full((max_len, B, n), UNSET_I, dtype=torch.int32, device="cuda"),
                lp=torch.full((max_len, B, n), UNSET_F, dtype=torch.float32, device="cuda"),
                rank=torch.full((max_len, B), UNSET_I, dtype=torch.int32, device="cuda"))


def _top_after(logits, keys, st, temp, n, forced=None, max_len=2, s=0):
    """a real decode_step_end_logprob, then the top-n launch behind it -> (the step end's buffers, the three outputs)"""
    b = _finish(logits, keys, st, temp, forced, max_len, s)
    o = _outs(max_len, keys.shape[0], n)
    _ops().decode_top_logprobs(logits, st, b["ids"], b["step"], o["ids"], o["lp"], o["rank"], temperature=temp, forced_ids=forced)
    return b, o


def _fed_entries_equal(top_ids, top_lp, fed, lp):
    """wherever the fed token is one of the n, its entry carries the bits of the token's own log-probability; returns how many were"""
    hit = top_ids.long() == fed[:, None]
    assert (hit.sum(-1) <= 1).all()
    rows = hit.any(-1)
    assert torch.equal(top_lp[hit].view(torch.int32), lp[rows].view(torch.int32)), "fed token's entry differs from its own log-probability"
    return int(rows.sum())


# ----------------------------------------------------------------------------- 1. + 4. against the reference; fused == stand-alone
@pytest.mark.parametrize("temp", [0.0, 0.7, 1.5])
@pytest.mark.parametrize("V", [40, 330, 4112])        # 2.5 tiles; a ragged last tile; more tiles than one pass of 256 threads
@pytest.mark.parametrize("kind", ["bf16", "fp8", "z13"])
def test_kernel_against_reference(kind, V, temp):
    ops = _ops()
    worst, hits = 0.0, 0
    for M in (1, 8, 64):
        logits, keys, st = _case(kind, V, M, temp)
        for n in (1, 5, 20):
            b, o = _top_after(logits, keys, st, temp, n)
            fed = b["ids"]
            want_ids, want_lp, want_rank = R.top(logits, n, temp, fed.cpu())
            assert torch.equal(o["ids"][0].long().cpu(), want_ids), f"M={M} n={n}: ids"
            assert torch.equal(o["rank"][0].long().cpu(), want_rank), f"M={M} n={n}: rank"
            worst = max(worst, R.logprobs_close(o["lp"][0], want_lp, 1e30))
            hits += _fed_entries_equal(o["ids"][0], o["lp"][0], fed, b["lp"][0])
            assert (o["ids"][1] == UNSET_I).all() and (o["lp"][1] == UNSET_F).all() and (o["rank"][1] == UNSET_I).all()   # only row s
            if not temp:
                assert torch.equal(o["ids"][0, :, 0].long(), b["pred"][0]) and (o["rank"][0] == 1).all()
            # the stand-alone entry: the same ids and ranks, its fed entries those of token_logprob
            a_ids, a_lp, a_rank = ops.top_logprobs(logits, fed, n, temp)
            assert torch.equal(a_ids, o["ids"][0]) and torch.equal(a_rank, o["rank"][0]), f"M={M} n={n}: stand-alone"
            worst = max(worst, R.logprobs_close(a_lp, want_lp, 1e30))
            _fed_entries_equal(a_ids, a_lp, fed, ops.token_logprob(logits, fed, temp))
    print(f"top logprobs {kind} V={V} T={temp}: largest |error| {worst:.3g}; fed token inside the n in {hits} rows")
    assert worst <= BOUND and (temp or hits == 3 * (1 + 8 + 64))


# ----------------------------------------------------------------------------- 2. crafted rows
@functools.lru_cache(maxsize=None)
def _zero_lin(V):
    return _ops().PackedLinear.from_weight(torch.zeros((V, 32), dtype=BF16, device="cuda"))


def _stored(rows, temp):
    """the rows as an lm_head call stores them: x = 0, W = 0, the rows as the residual -> (logits, keys, statistics)"""
    ops = _ops()
    M, V = rows.shape
    nt = (V + 15) // 16
    out = rows.cuda().clone()
    keys = torch.zeros((M, nt), dtype=torch.int64, device="cuda")
    st = torch.full((M, nt, 2), 7.0, dtype=torch.float32, device="cuda")
    ops.gemm(torch.zeros((M, 32), dtype=BF16, device="cuda"), _zero_lin(V), out=out, argmax_partial=keys, lse_partial=st,
             sample=(temp, SEED, None) if temp else None, residual=out)
    assert torch.equal(torch.nan_to_num(out.float().cpu(), nan=12345.0), torch.nan_to_num(rows.float(), nan=12345.0))
    return out, keys, st


def _both_entries(rows, temp, n, forced=None, ids=None):
    """the crafted rows through the fused entry (behind a real GEMM and step end) and, as written, through the stand-alone one; both
    against the reference.  Returns the fused outputs of row s = 0 and the step end's buffers."""
    ops = _ops()
    logits, keys, st = _stored(rows, temp)
    f = None if forced is None else torch.stack([forced, forced]).cuda()
    b, o = _top_after(logits, keys, st, temp, n, f)
    want = R.top(logits, n, temp, b["ids"].cpu())
    if forced is not None:          # a forced token outside the vocabulary: rank 0
        want[2][forced >= rows.shape[1]] = 0
    assert torch.equal(o["ids"][0].long().cpu(), want[0]) and torch.equal(o["rank"][0].long().cpu(), want[2])
    err = R.logprobs_close(o["lp"][0], want[1], BOUND)
    raw = rows.cuda()
    fed = b["ids"] if ids is None else ids.cuda()
    a_ids, a_lp, a_rank = ops.top_logprobs(raw, fed, n, temp)
    want_a = R.top(raw, n, temp, fed.cpu())
    assert torch.equal(a_ids.long().cpu(), want_a[0]) and torch.equal(a_rank.long().cpu(), want_a[2])
    err = max(err, R.logprobs_close(a_lp, want_a[1], BOUND))
    assert err <= BOUND, err
    return o, b, (a_ids, a_lp, a_rank), err


@pytest.mark.parametrize("temp", [0.0, R.T_COLLISION])
def test_crafted_rows(temp):
    worst = 0.0
    # V = 4112: all equal; the n-th value tied across the last tiles a sweep visits
    rows = torch.stack([R.row_all_equal(4112), R.row_straddle(), R.row_all_equal(4112, -3.0)])
    for n in (1, R.STRADDLE_N, 20):
        o, _, a, err = _both_entries(rows, temp, n)
        worst = max(worst, err)
        assert o["ids"][0, 0].tolist() == list(range(n)) and o["ids"][0, 2].tolist() == list(range(n))
        assert a[0][0].tolist() == list(range(n))
        if n == R.STRADDLE_N:
            assert o["ids"][0, 1].tolist() == [17, 2048, 3001, 3500, 3999] and a[0][1].tolist() == [17, 2048, 3001, 3500, 3999]
    # V = 330: +0 / -0 on top, the maximum in the last column of the ragged tile, the T = 1.5 collisions, tied and -inf columns
    rows = torch.stack([R.row_zeros_on_top(), R.row_max_in_last_column(), R.row_collision(), R.row_forced()])
    for n in (1, 3, 5, 20):
        o, _, a, err = _both_entries(rows, temp, n)
        worst = max(worst, err)
        if n == 3:
            assert o["ids"][0, 0].tolist() == [3, 7, 100] and a[0][0].tolist() == [3, 7, 100]
        assert int(o["ids"][0, 1, 0]) == 329 and int(a[0][1, 0]) == 329
        if n == 5:
            want = [5, 10, 20, 40, 200] if temp else [5, 20, 200, 10, 40]
            assert o["ids"][0, 2].tolist() == want and a[0][2].tolist() == want
    # V = 40: 30 columns of -inf and n = 20 - 10 finite entries, then 10 of -inf in column order; all equal at the smallest size
    rows = torch.stack([R.row_minus_inf(), R.row_all_equal(40)])
    o, _, a, err = _both_entries(rows, temp, 20)
    worst = max(worst, err)
    minus = [c for c in range(40) if rows[0, c] == float("-inf")][:10]
    for ids, lp in ((o["ids"][0, 0], o["lp"][0, 0]), (a[0][0], a[1][0])):
        assert ids[10:].tolist() == minus and torch.isfinite(lp[:10]).all() and (lp[10:] == float("-inf")).all()
    print(f"crafted rows T={temp}: largest |error| {worst:.3g}")


@pytest.mark.parametrize("temp", [0.0, 0.7])
def test_nan_row(temp):
    rows = torch.stack([R.row_forced(), R.row_collision(), R.row_forced(), R.row_zeros_on_top()])
    rows[2, 123] = float("nan")
    o, b, a, _ = _both_entries(rows, temp, 5)
    for ids, lp, rank in ((o["ids"][0], o["lp"][0], o["rank"][0]), a):
        assert ids[2].tolist() == [-1] * 5 and torch.isnan(lp[2]).all() and int(rank[2]) == 0
        assert (ids[[0, 1, 3]] >= 0).all() and torch.isfinite(lp[[0, 1, 3]]).all() and (rank[[0, 1, 3]] >= 1).all()
    assert math.isnan(float(b["lp"][0, 2]))


@pytest.mark.parametrize("temp", [0.0, 0.7])
def test_forced_tokens_and_ranks(temp):
    V = 330
    forced = torch.tensor([50, 60, 61, 300, 7, 100, V, V + 5, -1], dtype=torch.int64)
    ranks = [1, 2, 3, 4, 329, 330, 0, 0]
    rows = torch.stack([R.row_forced()] * len(forced))
    o, b, a, _ = _both_entries(rows, temp, 5, forced=forced, ids=forced)
    assert o["rank"][0, :8].tolist() == ranks and a[2].tolist() == ranks + [0]           # (stand-alone: an id of -1 is outside too)
    fed = b["ids"]
    assert torch.equal(fed[:6].cpu(), forced[:6]) and torch.equal(fed[6:], b["pred"][0, 6:])    # outside the vocabulary: never fed
    if not temp:
        assert int(o["rank"][0, 8]) == 1                 # the free-running row fed its own pick
    assert (b["lp"][0, 4:6] == float("-inf")).all() and torch.isnan(b["lp"][0, 6:8]).all()
    # the forced token's own entry, where it is among the 5: columns 50, 60, 61, 300
    assert _fed_entries_equal(o["ids"][0, :6], o["lp"][0, :6], fed[:6], b["lp"][0, :6]) == 4
    assert o["ids"][0, 0].tolist()[:4] == [50, 60, 61, 300]
    # with n = 20 on the V = 40 row a forced -inf column is one of the n: its entry is -inf like its own log-probability
    rows = torch.stack([R.row_minus_inf()] * 2)
    forced = torch.tensor([2, 39], dtype=torch.int64)
    o, b, a, _ = _both_entries(rows, temp, 20, forced=forced, ids=forced)
    assert int(o["rank"][0, 0]) == 12 and int(o["ids"][0, 0, 11]) == 2 and float(o["lp"][0, 0, 11]) == float("-inf")
    assert _fed_entries_equal(o["ids"][0], o["lp"][0], b["ids"], b["lp"][0]) == 2


def test_step_beyond_max_len_writes_nothing():
    logits, keys, st = _case("bf16", 330, 8, 0.0)
    b, o = _top_after(logits, keys, st, 0.0, 5, max_len=2, s=2)
    assert int(b["step"][0]) == 3
    assert (o["ids"] == UNSET_I).all() and (o["lp"] == UNSET_F).all() and (o["rank"] == UNSET_I).all()
    b, o = _top_after(logits, keys, st, 0.0, 5, max_len=2, s=1)          # the last row there is
    assert (o["ids"][0] == UNSET_I).all() and (o["rank"][1] == 1).all() and (o["ids"][1] >= 0).all()


# ----------------------------------------------------------------------------- 3. the determinism rule
@pytest.mark.parametrize("temp", [0.0, 0.7])
@pytest.mark.parametrize("kind", ["bf16", "z13"])
def test_bits_do_not_depend_on_the_batch(kind, temp):
    """row r alone and as row r of 8 and of 33 rows: the same bits in all three outputs (the rank of one forced token: the sampler's
    pick is keyed by the row index); the same call twice: the same bits"""
    N, r, n = 4112, 5, 20
    x = _x()

    def run(M):
        xs = x[r:r + 1] if M == 1 else x[:M]
        logits, keys, st = _gemm(kind, N, M, temp, x=xs)
        forced = torch.full((2, M), 123, dtype=torch.int64, device="cuda")
        _, o = _top_after(logits, keys, st, temp, n, forced)
        alone = _ops().top_logprobs(logits, forced[0].contiguous(), n, temp)
        i = 0 if M == 1 else r
        return [t[0, i:i + 1].clone() for t in (o["ids"], o["lp"], o["rank"])] + [t[i:i + 1].clone() for t in alone], o
    one = run(1)
    for M in (8, 33):
        many, again = run(M), run(M)
        for a, b in zip(one[0], many[0]):
            assert _same(a, b), f"row {r} alone vs in M={M}"
        assert all(_same(many[1][k], again[1][k]) for k in ("ids", "lp", "rank"))


# ----------------------------------------------------------------------------- 5. the per-row table
def _table(pars, seed=SEED):
    """umv_row_sampling rows, packed field by field: stream = the row index and draw = 0, the scalar calls' keying"""
    from unimedvl_amd import sampling
    t = np.zeros(len(pars), dtype=sampling.ROW_DTYPE)
    for i, (temp, top_k) in enumerate(pars):
        t[i] = (seed, 0, i, temp, top_k, 1.0, 0.0, 1.0, 0.0, 0.0)
    return sampling.to_tensor(t, "cuda")


def test_per_row_table_equals_scalar_calls():
    """mixed temperatures in one 16-row fragment (0, 0.7, 1.5, and two rows that truncate: the other merge order) equal, row by row,
    the scalar calls in which every row has that row's parameters"""
    ops = _ops()
    V, M, n = 330, 16, 5
    pars = [((0.0, 0.7, 1.5)[i % 3], 0) for i in range(M)]
    pars[4], pars[11] = (0.7, 5), (1.5, 3)
    lin = _lin("bf16", V)
    nt = (V + 15) // 16

    def run(rows=None, temp=0.0, top_k=0):
        b = _step_bufs(M, 2)                      # (max_len 2, step 0: the table's draw)
        out = torch.empty((M, V), dtype=BF16, device="cuda")
        keys = torch.zeros((M, nt), dtype=torch.int64, device="cuda")
        st = torch.zeros((M, nt, 2), dtype=torch.float32, device="cuda")
        o = _outs(2, M, n)
        if rows is not None:
            ops.gemm(_x()[:M], lin, out=out, argmax_partial=keys, lse_partial=st, sample_rows=rows)
            ops.decode_step_end_rows(b["slot"], b["pos"], b["kvl"], keys, b["ids"], b["in_ids"], b["pred"], b["step"], out, rows,
                                     lse_partial=st, logprobs=b["lp"])
        else:
            ops.gemm(_x()[:M], lin, out=out, argmax_partial=keys, lse_partial=st, sample=(temp, SEED, b["step"]) if temp else None)
            if top_k:
                ops.decode_step_end_truncated(b["slot"], b["pos"], b["kvl"], keys, b["ids"], b["in_ids"], b["pred"], b["step"], out, temp,
                                              SEED, top_k=top_k, lse_partial=st, logprobs=b["lp"])
            else:
                ops.decode_step_end_logprob(b["slot"], b["pos"], b["kvl"], keys, st, b["ids"], b["in_ids"], b["pred"], b["step"], out, b["lp"],
                                            temperature=temp)
        ops.decode_top_logprobs(out, st, b["ids"], b["step"], o["ids"], o["lp"], o["rank"], temperature=temp, sample_rows=rows,
                                truncated=bool(top_k))
        return b, o, out
    tb, to, tl = run(rows=_table(pars))
    for p in sorted(set(pars)):
        sb, so, sl = run(temp=p[0], top_k=p[1])
        mine = [i for i in range(M) if pars[i] == p]
        assert torch.equal(tb["ids"][mine], sb["ids"][mine]) and _same(tb["lp"][0, mine], sb["lp"][0, mine]), p
        for k in ("ids", "lp", "rank"):
            assert _same(to[k][0, mine], so[k][0, mine]), (p, k)
        want = R.top(sl[mine], n, p[0], sb["ids"][mine].cpu())
        assert torch.equal(so["ids"][0, mine].long().cpu(), want[0]) and torch.equal(so["rank"][0, mine].long().cpu(), want[2])
        assert _fed_entries_equal(to["ids"][0, mine], to["lp"][0, mine], tb["ids"][mine], tb["lp"][0, mine]) >= (len(mine) if not p[0] else 0)


# ----------------------------------------------------------------------------- 6. the engine
def _check_session_rows(sess_factory, steps, temp, n):
    """an eager session step by step against the reference on its own logits; returns (the session, the largest error)"""
    eager = sess_factory(use_graph=False)
    worst = 0.0
    for s in range(steps):
        eager.step(1)
        fed = eager.ids.cpu()
        want = R.top(eager.logits, n, temp, fed)
        assert torch.equal(eager.pred_top_ids[s].long().cpu(), want[0]), s
        assert torch.equal(eager.pred_rank[s].long().cpu(), want[2]), s
        worst = max(worst, R.logprobs_close(eager.pred_top_logprobs[s], want[1], BOUND))
        _fed_entries_equal(eager.pred_top_ids[s], eager.pred_top_logprobs[s], eager.ids, eager.pred_logprobs[s])
    return eager, worst


MODES = {"greedy": dict(), "top_p": dict(do_sample=True, temperature=0.7, seed=77, top_p=0.8),
         "penalty": dict(repetition_penalty=1.3, presence_penalty=0.25), "forced": "forced"}


@pytest.mark.parametrize("mode", list(MODES))
def test_session(model, mode):  # noqa: F811
    steps, n = 8, 5
    kw = MODES[mode]
    if kw == "forced":
        f = torch.randint(5, 290, (steps, 3), generator=torch.Generator().manual_seed(9))
        f[2:5, 1] = -1
        kw = dict(forced_ids=f)
    temp = kw.get("temperature", 0.0)
    with torch.no_grad():
        base = _session(model, steps, use_graph=True, logprobs=True, **kw)
        assert base.pred_top_ids is None and base.top_logprobs == 0
        base.step(steps)
        on = _session(model, steps, use_graph=True, top_logprobs=n, **kw)
        assert on.graph is not None and on.logprobs and on.pred_top_ids.shape == (steps, 3, n) and on.pred_rank.shape == (steps, 3)
        assert on.pred_top_ids.dtype == torch.int32 and on.pred_top_logprobs.dtype == torch.float32 and on.pred_rank.dtype == torch.int32
        on.step(steps)
        assert torch.equal(on.pred_ids, base.pred_ids) and torch.equal(on.in_ids, base.in_ids) and _same(on.pred_logprobs, base.pred_logprobs)
        assert all(torch.equal(a, b) for a, b in zip(_kv(on, steps), _kv(base, steps)))
        eager, worst = _check_session_rows(lambda **g: _session(model, steps, top_logprobs=n, **kw, **g), steps, temp, n)
        assert torch.equal(eager.pred_ids, on.pred_ids)
        for a, b in ((eager.pred_top_ids, on.pred_top_ids), (eager.pred_top_logprobs, on.pred_top_logprobs), (eager.pred_rank, on.pred_rank)):
            assert _same(a, b)                              # graph replay == eager
        if mode == "greedy":
            assert (on.pred_rank == 1).all() and torch.equal(on.pred_top_ids[:, :, 0].long(), on.pred_ids)
    print(f"session top_logprobs {mode}: largest |error| {worst:.3g}")
    assert worst <= BOUND
    on.rewind_outputs()
    assert int(on.step_idx.max()) == 0


def test_session_banned_columns(model):  # noqa: F811
    """under a logit bias of -inf the alternatives are those of the ADJUSTED logits: a banned column never stands above a finite one"""
    steps, n = 6, 20
    with torch.no_grad():
        free = _session(model, steps, use_graph=True, top_logprobs=n)
        free.step(steps)
        banned = sorted({int(t) for t in free.pred_top_ids[0, :, :3].flatten()})        # what every sample liked best at step 0
        bias = {t: float("-inf") for t in banned}
        mk = lambda **g: _session(model, steps, top_logprobs=n, logit_bias=bias, repetition_penalty=1.2, **g)   # noqa: E731
        eager, worst = _check_session_rows(mk, steps, 0.0, n)
        on = mk(use_graph=True)
        on.step(steps)
    assert _same(on.pred_top_logprobs, eager.pred_top_logprobs) and torch.equal(on.pred_top_ids, eager.pred_top_ids)
    assert torch.isfinite(on.pred_top_logprobs).all()                                   # the vocabulary has more than n finite columns
    assert not np.isin(on.pred_top_ids.cpu().numpy(), banned).any()
    assert worst <= BOUND


def test_generate_text_chat_score(model):  # noqa: F811
    from oracle.toy_tokenizer import ToyTokenizer
    from unimedvl_amd.bagel import TopLogprobs
    n = 4

    def run(**kw):
        cache, gi = _ctx(model)
        return model.generate_text(past_key_values=cache, max_length=8, **gi, **kw)
    ids0, lp0 = run(return_logprobs=True)
    ids, lp, top = run(top_logprobs=n)
    assert isinstance(top, TopLogprobs) and torch.equal(ids, ids0) and _same(lp, lp0)
    rows = ids.shape[0]
    assert top.ids.shape == (rows, 3, n) and top.logprobs.shape == (rows, 3, n) and top.rank.shape == (rows, 3)
    assert torch.equal(top.ids[:-1, :, 0].long(), ids[1:]) and (top.rank == 1).all() and _same(top.logprobs[:, :, 0], lp)
    ids2, logits, lp2, top2 = run(return_logits=True, return_logprobs=True, top_logprobs=n)
    assert torch.equal(ids2, ids) and all(_same(a, b) for a, b in zip(top2, top))         # eager == graph
    for s in range(rows):
        want = R.top(logits[s], n, 0.0)
        assert torch.equal(top.ids[s].long().cpu(), want[0]) and R.logprobs_close(top.logprobs[s], want[1], BOUND) <= BOUND
    empty = model.generate_text(past_key_values=_ctx(model)[0], max_length=0, top_logprobs=n, **_ctx(model)[1])
    assert empty[0].shape == (0, 3) and empty[2].ids.shape == (0, 3, n) and empty[2].rank.shape == (0, 3)
    with pytest.raises(ValueError, match="top_logprobs"):
        run(top_logprobs=21)
    with pytest.raises(ValueError, match="speculative|draft_len"):
        run(top_logprobs=n, draft_len=2)
    # chat and score
    tok = ToyTokenizer(NEW_TOKEN_IDS)
    ident = lambda x: x   # noqa: E731
    img = torch.randn(3, 28, 42, generator=torch.Generator().manual_seed(2)).clamp(-1, 1)
    prompt = "17 23 5"
    answer, own, own_lp = model.chat(tok, NEW_TOKEN_IDS, ident, [img], prompt, max_length=6, return_logprobs=True)
    answer2, own2, own_lp2, ctop = model.chat(tok, NEW_TOKEN_IDS, ident, [img], prompt, max_length=6, top_logprobs=n)
    assert (answer2, own2, own_lp2) == (answer, own, own_lp) and len(ctop.ids) == len(ctop.logprobs) == len(ctop.rank) == len(own) >= 1
    assert [t[0] for t in ctop.ids] == own and [v[0] for v in ctop.logprobs] == own_lp and ctop.rank == [1] * len(own)
    cands = [own, [7, 8], [9, 10, 11]]
    plain = model.score(tok, NEW_TOKEN_IDS, ident, [img], prompt, cands)
    res = model.score_top_logprobs(tok, NEW_TOKEN_IDS, ident, [img], prompt, cands, top_logprobs=n)
    ranks_only = model.score_top_logprobs(tok, NEW_TOKEN_IDS, ident, [img], prompt, cands)
    for c, p, r, r0 in zip(cands, plain, res, ranks_only):
        assert "token_ranks" not in p and {k: r[k] for k in p} == p and r0["token_ranks"] == r["token_ranks"] and "top_logprobs" not in r0
        assert len(r["token_ranks"]) == len(r["top_logprobs"]) == len(c) + 1 and all(len(t) == n for t in r["top_logprobs"])
        for t, v, rk, alts in zip(r["token_ids"], r["token_logprobs"], r["token_ranks"], r["top_logprobs"]):
            assert rk >= 1 and ((t, v) in alts) == (rk <= n) and (rk > n or alts[rk - 1] == (t, v))
    # the candidate that IS the greedy answer: every token first; its alternatives those of the free-running chat (1 row against 3)
    assert res[0]["token_ranks"][:len(own)] == [1] * len(own)
    assert [[i for i, _ in t] for t in res[0]["top_logprobs"][:len(own)]] == ctop.ids
    assert [[v for _, v in t] for t in res[0]["top_logprobs"][:len(own)]] == ctop.logprobs


@pytest.mark.parametrize("per_request", [False, True], ids=["batcher_wide", "per_request"])
@pytest.mark.parametrize("paged", [False, True], ids=["slab", "paged"])
def test_batcher(model, paged, per_request):  # noqa: F811
    """every request's alternatives and ranks equal those of the same request served alone in a one-slot batcher, cut where its tokens are"""
    from oracle.toy_tokenizer import ToyTokenizer
    from unimedvl_amd.sampling import SamplingParams
    from unimedvl_amd.serving import ContinuousBatcher
    tok = ToyTokenizer(NEW_TOKEN_IDS)
    reqs = _requests(5)
    budgets = [6, 3, 6, 5, 2]
    ident = lambda x: x   # noqa: E731
    samp = [None] * 5
    if per_request:          # (a request's key is its own seed, stream 0 and draw counter: the same alone and among others)
        samp = [None, SamplingParams(do_sample=True, temperature=0.7, seed=5), SamplingParams(do_sample=True, temperature=1.5, top_k=4, seed=6),
                SamplingParams(repetition_penalty=1.3), None]

    def serve(which, slots):
        srv = ContinuousBatcher(model, tok, NEW_TOKEN_IDS, ident, slots=slots, max_context=256, max_new_tokens=8, check_every=4,
                                paged=paged, top_logprobs=3, per_request_sampling=per_request, **(dict(seed=9) if per_request else {}))
        rids = [srv.submit(*reqs[i], max_new_tokens=budgets[i], **(dict(sampling=samp[i]) if per_request else {})) for i in which]
        return srv, rids, srv.run()
    srv, rids, got = serve(range(5), 3)
    assert sorted(srv.top_logprobs) == sorted(srv.ranks) == sorted(srv.logprobs) == sorted(rids)
    for i, rid in enumerate(rids):
        one, (r1,), alone = serve([i], 1)
        assert got[rid] == alone[r1], i
        assert len(srv.ranks[rid]) == len(srv.top_logprobs[rid]) == len(srv.logprobs[rid]) == len(one.logprobs[r1]) <= budgets[i]
        assert srv.ranks[rid] == one.ranks[r1] and srv.top_logprobs[rid] == one.top_logprobs[r1] and srv.logprobs[rid] == one.logprobs[r1], i
        assert all(len(t) == 3 for t in srv.top_logprobs[rid])
        if samp[i] is None or not samp[i].do_sample:
            assert all(r == 1 for r in srv.ranks[rid]) or samp[i] is not None


# ----------------------------------------------------------------------------- 7. refusals
def test_refusals(model):  # noqa: F811
    import ctypes as C
    from unimedvl_amd import _lib
    ops = _ops()
    lib = _lib.load()
    V, M = 40, 2
    logits = torch.zeros((M, V), dtype=BF16, device="cuda")
    ids = torch.zeros(M, dtype=torch.int64, device="cuda")
    step = torch.ones(M, dtype=torch.int64, device="cuda")
    st = torch.zeros((M, 3, 2), dtype=torch.float32, device="cuda")
    o = _outs(2, M, 20)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731

    def alone(n, ti=o["ids"], tl=o["lp"], rk=o["rank"]):
        return lib.umv_top_logprobs_bf16(p(logits), V, p(ids), M, V, 0.0, n, p(ti), p(tl), p(rk), None)

    def fused(n, ti=o["ids"], tl=o["lp"], rk=o["rank"], order=0):
        return lib.umv_decode_top_logprobs(p(logits), V, V, p(st), 3, 0.0, None, order, p(ids), p(step), None, M, 2, n, p(ti), p(tl), p(rk), None)
    for call in (alone, fused):
        for bad in (dict(n=0), dict(n=21), dict(n=5, ti=None), dict(n=5, tl=None), dict(n=5, rk=None)):
            assert call(**bad) == -1 and lib.umv_last_error().decode(), bad              # UMV_ERR_ARG with a message
    assert fused(5, order=7) == -1 and "merge_order" in lib.umv_last_error().decode()
    small = torch.zeros((M, 12), dtype=BF16, device="cuda")
    assert lib.umv_top_logprobs_bf16(p(small), 12, p(ids), M, 12, 0.0, 13, p(o["ids"]), p(o["lp"]), p(o["rank"]), None) == -1       # n > V
    assert "at most V" in lib.umv_last_error().decode()
    torch.cuda.synchronize()
    assert (o["ids"] == UNSET_I).all() and (o["rank"] == UNSET_I).all()                # a refused call wrote nothing
    with pytest.raises(_lib.UmvError, match="n must be"):
        ops.top_logprobs(logits, ids, 0)
    with pytest.raises(_lib.UmvError, match="n must be"):
        ops.decode_top_logprobs(logits, st, ids, step, torch.zeros((2, M, 21), dtype=torch.int32, device="cuda"),
                                torch.zeros((2, M, 21), dtype=torch.float32, device="cuda"), o["rank"])
    with pytest.raises(ValueError, match="top_logprobs"):
        _session(model, 4, use_graph=False, top_logprobs=21)
    from unimedvl_amd.serving import ContinuousBatcher
    with pytest.raises(ValueError, match="top_logprobs"):
        ContinuousBatcher(model, None, NEW_TOKEN_IDS, None, slots=1, top_logprobs=21)
    from unimedvl_amd.speculative import SpeculativeDecodeSession
    cache, gi = _ctx(model)
    with pytest.raises(ValueError, match="greedy only"):
        SpeculativeDecodeSession(model.language_model, cache, gi["packed_start_tokens"], gi["packed_query_position_ids"], 4, 2, top_logprobs=3)
