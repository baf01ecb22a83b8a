"""Beam search decode (include/unimedvl_hip.h, "beam search decode") at kernel level.
  umv_beam_candidates   ids exact against tests/top_logprobs_ref.py, log-probabilities within 1e-4 of fp64, and bit-equal to
                        umv_decode_top_logprobs on the same rows.
  umv_beam_step_end     six chained steps per shape, fed the device's own candidate lists, held to tests/beam_ref.py on EVERY output
                        word, bit for bit; crafted candidate lists for every branch, each asserted reached.
  umv_beam_kv_copy      with the step end's table rewrite on a real fork: after every step each row's logical K and V^T, gathered
                        through the table, are the Python permutation of the sequences, and no page outside the fork's spares changed."""
import functools

import numpy as np
import pytest
import torch

import beam_ref as R
import top_logprobs_ref as T
from test_logprob_gpu import BOUND, K as HID, _gemm, _ops, _same

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
P = 256
SHAPES = [(1, 2), (1, 4), (3, 3), (8, 8), (6, 10)]
VS = [330, 4112]


@functools.lru_cache(maxsize=None)
def _rows(V, R_, step=0):
    """logits and statistics of R_ rows, different for every step: (logits, lse)"""
    x = torch.randn(R_, HID, generator=torch.Generator().manual_seed(100 + step)).to(BF16).cuda()
    logits, _, st = _gemm("bf16", V, R_, 0.0, x=x)
    return logits, st


def _candidates(V, Rn, n, step=0):
    ops = _ops()
    logits, st = _rows(V, Rn, step)
    ids = torch.full((Rn, n), -3, dtype=torch.int32, device="cuda")
    lp = torch.full((Rn, n), 9.0, dtype=torch.float32, device="cuda")
    ops.beam_candidates(logits, st, ids, lp, torch.zeros(Rn, dtype=torch.int32, device="cuda"))
    return logits, st, ids, lp


# ----------------------------------------------------------------------------- candidates
@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("B,K", SHAPES)
def test_candidates(V, B, K):
    ops = _ops()
    Rn, n = B * K, 2 * K
    logits, st, ids, lp = _candidates(V, Rn, n)
    want_ids, want_lp, _ = T.top(logits.cpu(), n)
    assert torch.equal(ids.cpu().long(), want_ids)
    worst = T.logprobs_close(lp, want_lp, BOUND)
    print(f"candidates V={V} B={B} K={K}: max |lp - fp64| = {worst:.3g}")
    assert worst <= BOUND
    # the same rows through the top-n launch behind a greedy step end: the same bits
    top_ids = torch.zeros((1, Rn, n), dtype=torch.int32, device="cuda")
    top_lp = torch.zeros((1, Rn, n), dtype=torch.float32, device="cuda")
    rank = torch.zeros((1, Rn), dtype=torch.int32, device="cuda")
    ops.decode_top_logprobs(logits, st, torch.zeros(Rn, dtype=torch.int64, device="cuda"), torch.ones(Rn, dtype=torch.int64, device="cuda"),
                            top_ids, top_lp, rank)
    assert _same(top_ids[0], ids) and _same(top_lp[0], lp)


def _host_stats(rows):
    """the per-tile statistics (m_t, s_t) of crafted rows, on the host: a tile of -inf only is (-inf, 0), a NaN makes its s_t NaN"""
    M, V = rows.shape
    nt = (V + 15) // 16
    y = torch.full((M, nt * 16), float("-inf"))
    y[:, :V] = rows.float()
    tiles = y.view(M, nt, 16)
    m = tiles.max(-1).values
    ref = torch.where(torch.isinf(m) & (m < 0), torch.zeros_like(m), m)
    return torch.stack([m, torch.exp(tiles - ref[..., None]).sum(-1)], -1).contiguous().cuda()


def test_candidates_minus_inf_and_nan_rows():
    ops = _ops()
    rows = torch.stack([T.row_minus_inf(40), T.row_all_equal(40), T.row_minus_inf(40)])
    rows[2, 5] = float("nan")
    logits, st = rows.cuda(), _host_stats(rows)
    ids = torch.zeros((3, 20), dtype=torch.int32, device="cuda")
    lp = torch.zeros((3, 20), dtype=torch.float32, device="cuda")
    ops.beam_candidates(logits, st, ids, lp, torch.zeros(3, dtype=torch.int32, device="cuda"))
    want_ids, want_lp, _ = T.top(rows, 20)
    assert torch.equal(ids.cpu().long(), want_ids) and (ids[2] == -1).all() and torch.isnan(lp[2]).all()
    assert T.logprobs_close(lp, want_lp, BOUND) <= BOUND and torch.isinf(lp[0]).any()
    assert ids[1].tolist() == list(range(20))             # identical values: the lower column first


def test_candidates_refusals():
    ops = _ops()
    from unimedvl_amd._lib import UmvError
    logits, st = _rows(330, 4)
    good = dict(cand_ids=torch.zeros((4, 6), dtype=torch.int32, device="cuda"), cand_lp=torch.zeros((4, 6), dtype=torch.float32, device="cuda"),
                rank=torch.zeros(4, dtype=torch.int32, device="cuda"))
    for bad in (dict(cand_ids=torch.zeros((4, 5), dtype=torch.int32, device="cuda"), cand_lp=torch.zeros((4, 5), dtype=torch.float32, device="cuda")),
                dict(cand_ids=torch.zeros((4, 22), dtype=torch.int32, device="cuda"), cand_lp=torch.zeros((4, 22), dtype=torch.float32, device="cuda")),
                dict(cand_lp=torch.zeros((4, 6), dtype=torch.float64, device="cuda")), dict(rank=torch.zeros(3, dtype=torch.int32, device="cuda"))):
        with pytest.raises(UmvError):
            ops.beam_candidates(logits, st, **{**good, **bad})


# ----------------------------------------------------------------------------- the step end against beam_ref
class Harness:
    """B requests of K beams on the device and in beam_ref, word for word"""

    def __init__(self, B, K, max_len, eos, length_penalty, early):
        ops = _ops()
        self.ops, self.B, self.K, self.max_len, self.eos, self.early = ops, B, K, max_len, eos, early
        Rn = B * K
        dev = "cuda"
        self.len0 = [250 + b + P * (b % 2) for b in range(B)]          # a prompt that ends inside page 0 or page 1; 256 is crossed
        self.j0 = [n // P for n in self.len0]
        self.st = ops.BeamState(B, K, max_len, dev, length_penalty)
        self.slot = torch.tensor(self.len0, dtype=torch.int32).repeat_interleave(K).to(dev)
        self.pos = self.slot + 7
        self.kvl = self.slot + 1
        self.ids = torch.full((Rn,), -5, dtype=torch.int64, device=dev)
        self.step = torch.zeros(Rn, dtype=torch.int64, device=dev)
        self.NP, self.stride = 2, 8
        own = 100 + torch.arange(Rn * self.NP * 2, dtype=torch.int32).reshape(Rn, self.NP, 2)
        table = torch.zeros((Rn, self.stride), dtype=torch.int32)
        for r in range(Rn):
            j = self.j0[r // K]
            table[r, :j] = 50 + r // K
            table[r, j:j + self.NP] = own[r, :, 0]
        self.own, self.table, self.j0_dev = own.to(dev), table.to(dev), torch.tensor(self.j0, dtype=torch.int32).to(dev)
        self.ref = [R.Request(K, max_len, eos, length_penalty, early) for _ in range(B)]
        self.mirror = self.words()
        self.reached = set()

    def words(self):
        st = self.st
        return {k: v.cpu().clone() for k, v in dict(slot=self.slot, pos=self.pos, kvl=self.kvl, ids=self.ids, step=self.step, scores=st.scores,
                                                   tok=st.beam_tok, parent=st.beam_parent, lp=st.beam_lp, fin_f=st.fin_f, fin_i=st.fin_i,
                                                   hdr=st.hdr, copies=st.copies, table=self.table).items()}

    def set_scores(self, b, scores):
        self.st.scores[b * self.K:(b + 1) * self.K] = torch.tensor(scores, dtype=torch.float32, device="cuda")
        self.ref[b].scores[:] = np.asarray(scores, dtype=np.float32)
        self.mirror["scores"][b * self.K:(b + 1) * self.K] = torch.tensor(scores, dtype=torch.float32)

    def run(self, cand_ids=None, cand_lp=None):
        """one step end; cand_*: crafted lists [R][2K] (default: what the candidates launch left in the state).  Compares every word."""
        ops, st, K, B = self.ops, self.st, self.K, self.B
        if cand_ids is not None:
            st.cand_ids.copy_(torch.as_tensor(cand_ids, dtype=torch.int32).reshape(B * K, 2 * K))
            st.cand_lp.copy_(torch.as_tensor(cand_lp, dtype=torch.float32).reshape(B * K, 2 * K))
        ids, lps = st.cand_ids.cpu().numpy(), st.cand_lp.cpu().numpy()
        ops.beam_step_end(self.slot, self.pos, self.kvl, self.ids, self.step, st, self.table, self.own, self.j0_dev, self.eos, self.early)
        m = self.mirror
        own = self.own.cpu().numpy()
        for b, req in enumerate(self.ref):
            rows = slice(b * K, (b + 1) * K)
            t = req.steps
            out = req.step_end(ids[rows], lps[rows])
            self.reached |= req.reached
            if out is None:
                continue                                  # done: no word of the mirror changes
            toks, parents, totals, lp = out
            L = int(m["slot"][b * K]) + 1
            new, copies = R.kv_plan(m["table"][rows].numpy(), own[rows], self.j0[b], L, parents, done_now=bool(req.done))
            m["table"][rows] = torch.from_numpy(new)
            m["copies"][rows, :3] = torch.from_numpy(copies)
            m["ids"][rows] = torch.from_numpy(toks)
            m["tok"][t, rows], m["parent"][t, rows], m["lp"][t, rows] = torch.from_numpy(toks).int(), torch.from_numpy(parents), torch.from_numpy(lp)
            m["scores"][rows] = torch.from_numpy(totals)
            for k in ("slot", "pos", "kvl", "step"):
                m[k][rows] += 1
            m["fin_f"][b], m["fin_i"][b] = torch.from_numpy(req.fin_f), torch.from_numpy(req.fin_i)
            m["hdr"][b] = torch.tensor([req.n_fin, req.n_ever, req.done, 0], dtype=torch.int32)
        got = self.words()
        for k in m:
            assert _same(got[k], m[k]), (k, got[k], m[k])


@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("B,K", SHAPES)
def test_step_end_six_chained_steps(V, B, K):
    ops = _ops()
    _, _, ids0, _ = _candidates(V, B * K, 2 * K, 0)
    eos = int(ids0[0, 1])                                 # a token the rows do rank high: hypotheses finish
    for early, lp in ((False, 1.0), (True, 2.0)):
        h = Harness(B, K, 6, eos, lp, early)
        for step in range(6):
            logits, st = _rows(V, B * K, step)
            ops.beam_candidates(logits, st, h.st.cand_ids, h.st.cand_lp, h.st.rank)
            h.run()
        assert {"dead_beam", "max_length"} <= h.reached or any(r.done for r in h.ref)


def _lists(K, rows):
    """crafted candidate lists: rows = per beam a list of (token, probability); padded to 2K with distinct unlikely tokens"""
    ids = np.zeros((K, 2 * K), dtype=np.int32)
    lp = np.zeros((K, 2 * K), dtype=np.float32)
    for i, row in enumerate(rows):
        row = list(row) + [(200 + 20 * i + j, 1e-9) for j in range(2 * K - len(row))]
        ids[i], lp[i] = [t for t, _ in row], np.log(np.array([p for _, p in row], dtype=np.float32))
    return ids, lp


@pytest.mark.parametrize("length_penalty", [0.0, 1.0, 2.0])
def test_step_end_crafted_cases(length_penalty):
    K, eos = 2, 7
    h = Harness(1, K, 8, eos, length_penalty, False)
    first = _lists(K, [[(7, 0.4), (1, 0.3), (2, 0.2), (3, 0.1)]] * 2)
    h.run(*first)                                         # the first step: beam 1 is at -inf; the end token first in the order
    assert {"dead_beam", "end_top", "append"} <= h.reached and h.mirror["parent"][0].tolist() == [0, 0]
    second = _lists(K, [[(1, 0.6), (7, 0.3), (2, 0.05), (3, 0.05)], [(7, 0.3), (4, 0.25), (5, 0.25), (6, 0.2)]])
    h.run(*second)                                        # end token at r = 1 (finished) and at r = 2 (skipped)
    assert "end_skipped" in h.reached and int(h.mirror["hdr"][0, 0]) == 2
    h.set_scores(0, [0.0, 0.0])
    h.run(*second)                                        # a tie between beam 0's end token and beam 1's: the lower beam first; replaced
    assert "replace" in h.reached
    h.st.fin_f[0, :, 0] = h.st.fin_f[0, :, 0].min()
    h.ref[0].fin_f[:, 0] = h.ref[0].fin_f[:, 0].min()
    h.mirror["fin_f"][0, :, 0] = h.mirror["fin_f"][0, :, 0].min()
    h.set_scores(0, [0.0, 0.0])
    h.run(*second)
    if length_penalty == 0.0:                             # the same total over norm = 1: equality, nothing replaced
        assert "equal_kept" in h.reached
    h.set_scores(0, [-100.0, -100.0])
    h.run(*second)                                        # the heuristic: the best live total is below the worst finished score
    assert "heuristic_done" in h.reached and int(h.mirror["hdr"][0, 2]) == 1
    h.run(*second)                                        # done: untouched
    assert "done_untouched" in h.reached


def test_step_end_identical_rows_minus_inf_and_early_stopping():
    K, eos = 3, 9
    h = Harness(2, K, 4, eos, 1.0, True)
    same = [(1, 0.25), (2, 0.25), (3, 0.25), (4, 0.125), (5, 0.125), (6, 0.0)]      # -inf columns: probability 0
    with np.errstate(divide="ignore"):
        ids, lp = _lists(K, [same] * K)
    h.run(np.concatenate([ids, ids]), np.concatenate([lp, lp]))
    h.set_scores(0, [-1.0, -1.0, -1.0])                   # identical rows, identical scores: beam 0's candidates come first
    h.set_scores(1, [-1.0, float("-inf"), -1.0])
    h.run(np.concatenate([ids, ids]), np.concatenate([lp, lp]))
    assert h.mirror["parent"][1].tolist() == [0, 0, 0, 0, 0, 0] and h.mirror["tok"][1, :3].tolist() == [1, 2, 3]
    assert np.isneginf(lp).any()
    ends = _lists(K, [[(9, 0.5), (1, 0.5)], [(9, 0.6), (2, 0.4)], [(9, 0.7), (3, 0.3)]])
    h.set_scores(0, [-1.0, -1.0, -1.0])
    h.run(np.concatenate([ends[0], ids]), np.concatenate([ends[1], lp]))            # three end tokens in front: the list fills, done
    assert int(h.mirror["hdr"][0, 2]) == 1 and int(h.mirror["hdr"][1, 2]) == 0 and "end_top" in h.reached
    assert h.mirror["copies"][:K, 2].tolist() == [0, 0, 0]
    h.run(np.concatenate([ends[0], ids]), np.concatenate([ends[1], lp]))            # request 0 untouched, request 1 at max_length
    assert {"done_untouched", "max_length"} <= h.reached and int(h.mirror["hdr"][1, 2]) == 1


# ----------------------------------------------------------------------------- the KV reorder on a real fork
PARENTS = [[0, 1, 2], [0, 0, 1], [1, 0, 2], [2, 2, 2], [0, 2, 1], [1, 1, 0]]       # identity, two children of one parent, swaps


@pytest.mark.parametrize("hd", [128, 72])
def test_kv_reorder(hd):
    ops = _ops()
    from unimedvl_amd.kvcache import PagedCache
    layers, nkv, B, K, prompt, steps = 2, 2, 2, 3, 250, 12
    Rn = B * K
    g = torch.Generator().manual_seed(hd)
    c = PagedCache(layers, pool_pages=40, max_context=2048)
    c.ensure_tokens([prompt] * B + [100], nkv, hd, "cuda")                  # a third segment: another request's pages
    for sl in c.pool.slabs:                                                 # every page of the pool holds something to corrupt
        sl.k.copy_(torch.randn(sl.k.shape, generator=g).to(BF16))
        sl.vt.copy_(torch.randn(sl.vt.shape, generator=g).to(BF16))
    c.lens = [prompt] * B + [100]
    tok_k = torch.randn(layers, Rn, prompt + steps + 1, nkv, hd, generator=g).to(BF16).cuda()      # what row r appends at slot s
    tok_v = torch.randn(layers, Rn, prompt + steps + 1, nkv, hd, generator=g).to(BF16).cuda()
    f = c.view_segments(0, B).fork_beams(K, steps + 2)
    private = set(f.beam_own.cpu().reshape(-1).tolist()) - {0}
    outside = [p for p in range(c.pool.npages) if p not in private]
    base = [(sl.k.clone(), sl.vt.clone()) for sl in c.pool.slabs]
    st = ops.BeamState(B, K, steps + 4, "cuda", 1.0)     # (never the last step: no hypothesis finishes, no request is done)
    slot = torch.full((Rn,), prompt, dtype=torch.int32, device="cuda")
    pos, kvl = slot.clone(), slot + 1
    ids, step = torch.zeros(Rn, dtype=torch.int64, device="cuda"), torch.zeros(Rn, dtype=torch.int64, device="cuda")
    pools = ops.beam_pool_pointers(f.pool.slabs)
    seqs = [[] for _ in range(Rn)]                       # a row's generated sequence: per slot the row that appended it
    table = f.pool.table
    for t in range(steps):
        L = prompt + t + 1
        tab = table.cpu()
        for r in range(Rn):                              # the append of umv_qkv_post: every row its own token at slot L - 1
            pg, s = int(tab[r, (L - 1) // P]), (L - 1) % P
            assert pg in private and sum(int(tab[o, (L - 1) // P]) == pg for o in range(Rn)) == 1, "invariant (a)"
            for l, sl in enumerate(f.pool.slabs):
                sl.k[pg, :, s, :] = tok_k[l, r, L - 1]
                sl.vt[pg, :, :, s] = tok_v[l, r, L - 1]
            seqs[r].append(r)
        parents = [PARENTS[(t + b) % len(PARENTS)] for b in range(B)]
        cand_ids = np.zeros((Rn, 2 * K), dtype=np.int32)
        cand_lp = np.full((Rn, 2 * K), -50.0, dtype=np.float32)
        for b in range(B):                               # child c is the c-th best candidate of the request and sits in its parent's list
            used = [0] * K
            for ch, p in enumerate(parents[b]):
                cand_lp[b * K + p, used[p]] = -0.1 * (ch + 1)
                used[p] += 1
            cand_ids[b * K:(b + 1) * K] = 10 + np.arange(K * 2 * K).reshape(K, 2 * K)
        st.cand_ids.copy_(torch.from_numpy(cand_ids))
        st.cand_lp.copy_(torch.from_numpy(cand_lp))
        st.scores.zero_()
        before = [(sl.k.clone(), sl.vt.clone()) for sl in c.pool.slabs]
        ops.beam_step_end(slot, pos, kvl, ids, step, st, table, f.beam_own, f.beam_j0, None, False)
        ops.beam_kv_copy(st.copies, pools, f.pool.slabs)
        assert st.beam_parent[t].cpu().reshape(B, K).tolist() == parents
        seqs = [list(seqs[(r // K) * K + parents[r // K][r % K]]) for r in range(Rn)]
        new, copies = table.cpu(), st.copies.cpu()
        # what changed: only the destinations of the copy list, all of them spares of this fork that no row named before the step
        dst = {int(d) for _, d, n, _ in copies.tolist() if n}
        assert dst <= private and not dst & set(tab.reshape(-1).tolist())
        assert all(n % 8 == 0 and L % P <= n <= P for _, _, n, _ in copies.tolist() if n)
        for l, sl in enumerate(c.pool.slabs):
            keep = [p for p in range(c.pool.npages) if p not in dst]
            assert torch.equal(sl.k[keep].view(torch.int16), before[l][0][keep].view(torch.int16)), "invariants (b), (c)"
            assert torch.equal(sl.vt[keep].view(torch.int16), before[l][1][keep].view(torch.int16))
            assert torch.equal(sl.k[outside].view(torch.int16), base[l][0][outside].view(torch.int16)), "invariant (d)"
            assert torch.equal(sl.vt[outside].view(torch.int16), base[l][1][outside].view(torch.int16))
        # every row's logical K and V^T through the table: the permuted sequences, bit for bit
        for r in range(Rn):
            for l, sl in enumerate(f.pool.slabs):
                pages = new[r, :L // P + 1].long().cuda()
                k = sl.k[pages].permute(1, 0, 2, 3).reshape(nkv, -1, hd)[:, :L]              # [nkv][L][hd]
                v = sl.vt[pages].permute(1, 2, 0, 3).reshape(nkv, hd, -1)[:, :, :L]          # [nkv][hd][L]
                src, at = torch.tensor(seqs[r]).cuda(), torch.arange(prompt, L).cuda()
                want_k, want_v = tok_k[l, src, at], tok_v[l, src, at]                            # [L - prompt][nkv][hd]
                assert torch.equal(k[:, prompt:].view(torch.int16), want_k.permute(1, 0, 2).contiguous().view(torch.int16)), (t, r, l)
                assert torch.equal(v[:, :, prompt:].view(torch.int16), want_v.permute(1, 2, 0).contiguous().view(torch.int16)), (t, r, l)
                ppage = c.pool.host_table[r // K][0]
                assert torch.equal(k[:, :prompt].view(torch.int16), base[l][0][ppage][:, :prompt].view(torch.int16))
                assert torch.equal(v[:, :, :prompt].view(torch.int16), base[l][1][ppage][:, :, :prompt].view(torch.int16))
    used = c.pages_in_use()
    f.release_all()
    assert c.pages_in_use() == used - len(private)
