"""Beam search decode (include/unimedvl_hip.h, "beam search decode"), the parts that need no GPU: tests/beam_ref.py - the plain-Python
form of the definition - held to HF's generate on a small random causal LM, to greedy decode and to exhaustive search; the page
accounting of PagedCache.fork_beams / release_all; the refused keyword combinations; the binding.
(The kernels and the engine are GPU tests: tests/test_beam_gpu.py, tests/test_beam_engine_gpu.py.)"""
import ctypes
import inspect
import itertools
import os
import re

import numpy as np
import pytest
import torch

import beam_ref as R
from unimedvl_amd import ops
from unimedvl_amd.kvcache import NaiveCache, PagedCache

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ops.KV_PAGE


# ----------------------------------------------------------------------------- the definition against HF's generate
@pytest.fixture(scope="module")
def hf_model():
    from transformers import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(7)
    cfg = LlamaConfig(vocab_size=48, hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, max_position_embeddings=128, pad_token_id=0, bos_token_id=1, eos_token_id=2)
    m = LlamaForCausalLM(cfg).float().eval()
    with torch.no_grad():
        for p in m.parameters():                         # random weights well away from a near-uniform softmax
            p.mul_(4.0)
    return m


def _hf_fn(model, prompt):
    def fn(prefixes):
        with torch.no_grad():
            ids = torch.tensor([prompt + list(p) for p in prefixes], dtype=torch.int64)
            return torch.log_softmax(model(ids).logits[:, -1, :].float(), -1).numpy()
    return fn


# (K, steps, prompt, end token): end tokens this model does emit, so that hypotheses finish before max_length, lists fill up and
# entries are replaced - and one it never emits (2)
HF_CASES = [(3, 10, [1, 5, 9, 11], 2), (3, 10, [1, 5, 9, 11], 37), (3, 10, [1, 5, 9, 11], 40), (4, 7, [1, 20, 21], 13),
            (4, 7, [1, 20, 21], 36), (2, 12, [1, 33], 36), (2, 12, [1, 33], 18)]


@pytest.mark.parametrize("length_penalty", [0.0, 1.0, 2.0])
@pytest.mark.parametrize("K,steps,prompt,eos", HF_CASES)
def test_beam_ref_is_hf_generate(hf_model, length_penalty, K, steps, prompt, eos):
    """sequences and sequences_scores of generate(num_beams=K, do_sample=False, early_stopping=True), all K returned"""
    out = hf_model.generate(torch.tensor([prompt]), num_beams=K, do_sample=False, early_stopping=True, length_penalty=length_penalty,
                            max_length=len(prompt) + steps, num_return_sequences=K, return_dict_in_generate=True, output_scores=True,
                            eos_token_id=eos, pad_token_id=0)
    req = R.search(_hf_fn(hf_model, prompt), K, steps, eos, length_penalty=length_penalty, early_stopping=True)
    hyps = req.hypotheses()
    assert len(hyps) == K == out.sequences.shape[0]
    for h, seq, score in zip(hyps, out.sequences.tolist(), out.sequences_scores.tolist()):
        gen = seq[len(prompt):]
        assert gen[:len(h["tokens"])] == h["tokens"], (h, gen)
        assert all(t == eos for t in gen[len(h["tokens"]):])                 # HF fills behind a hypothesis (pad id 0 counts as unset)
        assert abs(h["score"] - score) <= 1e-5 * max(1.0, abs(score)), (h["score"], score)


def test_hf_cases_end_hypotheses_before_max_length(hf_model):
    """the comparison above covers finished hypotheses, not only the offer at max_length"""
    early, reached = 0, set()
    for K, steps, prompt, eos in HF_CASES:
        req = R.search(_hf_fn(hf_model, prompt), K, steps, eos, length_penalty=1.0, early_stopping=True)
        early += sum(h["tokens"][-1] == eos and len(h["tokens"]) < steps for h in req.hypotheses())
        reached |= req.reached
    assert early >= 6 and {"end_top", "end_skipped", "append", "replace", "worse_kept", "max_length", "dead_beam"} <= reached, (early, reached)


def test_beam_ref_done_rules_follow_hf(hf_model):
    """early_stopping=False: the best hypothesis is HF's too (its heuristic: worst finished score >= best live total / current length)"""
    prompt, eos = [1, 5, 9, 11], 37
    for lp in (0.0, 1.0, 2.0):
        out = hf_model.generate(torch.tensor([prompt]), num_beams=3, do_sample=False, early_stopping=False, length_penalty=lp,
                                max_length=len(prompt) + 14, num_return_sequences=1, return_dict_in_generate=True, output_scores=True,
                                eos_token_id=eos, pad_token_id=0)
        best = R.search(_hf_fn(hf_model, prompt), 3, 14, eos, length_penalty=lp, early_stopping=False).hypotheses()[0]
        gen = out.sequences[0].tolist()[len(prompt):]
        assert gen[:len(best["tokens"])] == best["tokens"]
        assert abs(best["score"] - float(out.sequences_scores[0])) <= 1e-5 * max(1.0, abs(best["score"]))


# ----------------------------------------------------------------------------- toy models
def _toy(V, seed, eos_bias=0.0):
    """a model whose next-token distribution depends on the last two tokens: prefixes -> log-prob rows"""
    rng = np.random.default_rng(seed)
    tab = rng.normal(size=(V + 1, V + 1, V)).astype(np.float32) * 2.0
    tab[:, :, 0] += eos_bias

    def fn(prefixes):
        rows = []
        for p in prefixes:
            a, b = ([V, V] + list(p))[-2:]
            x = tab[a, b].astype(np.float64)
            rows.append((x - np.log(np.exp(x - x.max()).sum()) - x.max()).astype(np.float32))
        return np.stack(rows)
    return fn


def test_one_beam_with_early_stopping_is_greedy():
    V, eos, steps = 9, 0, 12
    for seed in range(6):
        fn = _toy(V, seed, eos_bias=0.5)
        greedy = []
        while len(greedy) < steps:
            greedy.append(int(np.argmax(fn([greedy])[0])))
            if greedy[-1] == eos:
                break
        req = R.search(fn, 1, steps, eos, early_stopping=True)
        assert req.hypotheses()[0]["tokens"] == greedy


def test_wide_beam_is_exhaustive_search():
    """V = 6, length 4, K >= V^3: nothing is pruned, so the best hypothesis is the best of all sequences (no end token: all of length 4).
    A wide beam needs more than the 2K own candidates no beam ever has: n_candidates = V."""
    V, T = 6, 4
    for seed, lp in ((0, 0.0), (1, 1.0), (2, 2.0)):
        fn = _toy(V, seed)
        best, best_score = None, -np.inf
        for seq in itertools.product(range(V), repeat=T):
            s = np.float32(0)
            for t in range(T):
                s = np.float32(s + fn([list(seq[:t])])[0][seq[t]])
            if s > best_score:
                best, best_score = list(seq), s
        req = R.search(fn, V ** 3, T, None, length_penalty=lp, n_candidates=V)
        h = req.hypotheses()[0]
        assert h["tokens"] == best and h["total"] == pytest.approx(float(best_score), abs=1e-5)
        assert h["score"] == pytest.approx(float(best_score) / T ** lp, rel=1e-6)


def test_crafted_step_end_cases_are_reached():
    """the branches of the step end, each asserted reached: dead beams at the first step, end tokens inside and outside the first K,
    replacement in a full list and none on equality, both done rules, a done request left untouched"""
    K, eos = 2, 7
    ids = np.array([[7, 1, 2, 3], [7, 4, 5, 6]], dtype=np.int32)
    req = R.Request(K, 8, eos, length_penalty=0.0, early_stopping=False)
    out = req.step_end(ids, np.log(np.array([[0.4, 0.3, 0.2, 0.1]] * 2, dtype=np.float32)))
    assert {"dead_beam", "end_top", "append"} <= req.reached and out[0].tolist() == [1, 2] and out[1].tolist() == [0, 0]
    # both beams alive: beam 0's end token is second in the order (finished, the list is full), beam 1's third (skipped); the best live
    # total is above the worst finished score: not done
    ids = np.array([[1, 7, 2, 3], [7, 4, 5, 6]], dtype=np.int32)
    lp = np.log(np.array([[0.6, 0.3, 0.05, 0.05], [0.3, 0.25, 0.25, 0.2]], dtype=np.float32))
    req.step_end(ids, lp)
    assert "end_skipped" in req.reached and req.n_fin == 2 and "heuristic_open" in req.reached and not req.done
    assert req.parent[1].tolist() == [0, 1] and req.tok[1].tolist() == [1, 4]
    # a full list: a better hypothesis replaces the worst; beam 0's end token ties with beam 1's best and comes first (lower beam)
    req.scores[:] = 0.0
    req.step_end(ids, lp)
    assert "replace" in req.reached and sorted(req.fin_f[:, 0].tolist()) == sorted(np.log(np.array([0.3, 0.4], dtype=np.float32)).tolist())
    # ... an equal one does not
    req.fin_f[:, 0] = req.fin_f[:, 0].min()
    req.scores[:] = 0.0
    n_ever = req.n_ever
    req.step_end(ids, lp)
    assert "equal_kept" in req.reached and req.n_ever == n_ever and not req.done
    # done by the heuristic, then untouched
    req.scores[:] = -100.0
    req.step_end(ids, lp)
    assert {"heuristic_done", "worse_kept"} <= req.reached and req.done
    before = (req.scores.copy(), req.fin_f.copy(), req.steps)
    assert req.step_end(ids, lp) is None and "done_untouched" in req.reached
    assert np.array_equal(before[0], req.scores) and np.array_equal(before[1], req.fin_f) and before[2] == req.steps
    # early stopping: done as soon as the list is full
    early = R.Request(1, 8, eos, early_stopping=True)
    early.step_end(np.array([[7, 1]], dtype=np.int32), np.log(np.array([[0.6, 0.4]], dtype=np.float32)))
    assert early.done and early.hypotheses()[0]["tokens"] == [7]


def test_kv_plan_keeps_the_invariants():
    """the reorder rule on a host model of the table: after every step the page a row appends to next is referenced by no other row,
    copies go from current pages to spares, and a row's logical page list is its parent's"""
    rng = np.random.default_rng(3)
    K, j0, NP, stride = 3, 1, 3, 8
    table = np.zeros((K, stride), dtype=np.int32)
    table[:, 0] = 5                                      # the shared prompt page
    own = np.arange(10, 10 + K * NP * 2, dtype=np.int32).reshape(K, NP, 2)
    table[:, j0:j0 + NP] = own[:, :, 0]
    content = {int(pg): [] for pg in own.reshape(-1)}    # page -> the tokens it holds, as (step, row that appended it)
    seqs = [[("prompt", i) for i in range(250)] for _ in range(K)]           # the partially filled prompt page came along
    for c in range(K):
        content[int(own[c, 0, 0])] = list(seqs[c])
    for step, L in enumerate(range(P + 250 + 1, P + 250 + 300)):
        slot = L - 1
        for c in range(K):                               # every row appends its token at `slot`
            pg = int(table[c, slot // P])
            assert sum(int(table[o, slot // P]) == pg for o in range(K)) == 1, "invariant (a)"
            del content[pg][slot % P:]
            content[pg].append((step, c))
            seqs[c].append((step, c))
        parents = [0, 0, 1] if step % 3 == 0 else ([1, 0, 2] if step % 3 == 1 else list(rng.integers(0, K, K)))
        new, copies = R.kv_plan(table, own, j0, L, parents)
        for c in range(K):
            src, dst, n = (int(v) for v in copies[c])
            if n:
                assert src in table[:, L // P] and dst not in table[:, L // P] and dst in own[c, L // P - j0] and n >= L % P
                content[dst] = list(content[src][:L % P])
        table = new
        seqs = [list(seqs[p]) for p in parents]
        for c in range(K):
            got = [t for j in range(j0, L // P + 1) for t in content[int(table[c, j])][:max(0, min(P, L - j * P))]]
            assert got == seqs[c][-len(got):] and len(got) == L - j0 * P, (step, c)


# ----------------------------------------------------------------------------- fork_beams / release_all
def _prompt_cache(lens, pool_pages=64):
    c = PagedCache(2, pool_pages=pool_pages, max_context=4096)
    c.ensure_tokens(lens, 1, 8, "cpu")
    for l, sl in enumerate(c.slabs):
        for s, n in enumerate(lens):
            for pos in range(n):
                pg = int(sl.table[s, pos // P])
                sl.k[pg, :, pos % P, :] = pos + 1000 * l + 100000 * s
                sl.vt[pg, :, :, pos % P] = pos + 1000 * l + 100000 * s
    c.lens = list(lens)
    return c


def test_fork_beams_page_accounting():
    lens, K, horizon = [300, 256, 10], 3, 250
    c = _prompt_cache(lens)
    before = c.pages_in_use()
    assert before == 2 + 1 + 1
    f = c.fork_beams(K, horizon)
    npg = [(n + horizon - 1) // P - n // P + 1 for n in lens]
    assert npg == [2, 1, 2] and c.pages_in_use() == before + 2 * K * sum(npg)
    assert f.lens == [300] * 3 + [256] * 3 + [10] * 3 and f.beam_j0.tolist() == [1, 1, 0] and tuple(f.beam_own.shape) == (9, 2, 2)
    t = f.pool.table
    for b, n in enumerate(lens):
        for r in range(b * K, (b + 1) * K):
            assert t[r, :n // P].tolist() == c.pool.host_table[b][:n // P]                         # the full prompt pages, shared
            assert int(t[r, n // P]) == int(f.beam_own[r, 0, 0]) and c.pool.refs[int(t[r, n // P])] == 1
            for l in range(2):                                                                  # the partial page came along
                assert torch.equal(f.slabs[l].k[int(t[r, n // P]), :, :n % P], c.slabs[l].k[c.pool.host_table[b][n // P], :, :n % P]) \
                    if n % P else True
    private = f.beam_own[f.beam_own > 0].tolist()
    assert len(private) == len(set(private)) == 2 * K * sum(npg) and not set(private) & {p for row in c.pool.host_table for p in row}
    assert all(c.pool.refs[p] == 1 + K for p in c.pool.host_table[0][:1])
    # a decode session's own reservation finds every page in place
    f.ensure_tokens([n + horizon for n in f.lens], 1, 8, "cpu")
    assert c.pages_in_use() == before + 2 * K * sum(npg)
    keys = [c.packed_keys(l).clone() for l in range(2)]
    f.release_all()
    assert c.pages_in_use() == before and all(r == 1 for r in (c.pool.refs[p] for row in c.pool.host_table for p in row))
    assert int(f.pool.table.abs().sum()) == 0
    for l in range(2):
        assert torch.equal(c.packed_keys(l), keys[l])
    f2 = c.fork_beams(2, 600)                             # the pages can be taken again
    f2.release_all()
    assert c.pages_in_use() == before


def test_refused_fork_takes_no_page():
    c = _prompt_cache([300, 40], pool_pages=20)
    before, free = c.pages_in_use(), list(c.pool.free)
    with pytest.raises(RuntimeError, match="exhausted"):
        c.fork_beams(4, 300)                              # 2 * 4 * (2 + 2) = 32 pages
    with pytest.raises(ValueError, match="reach"):
        c.fork_beams(2, 5000)
    with pytest.raises(ValueError):
        c.fork_beams(0, 10)
    assert c.pages_in_use() == before and c.pool.free == free and all(c.pool.refs[p] == 1 for row in c.pool.host_table for p in row)


# ----------------------------------------------------------------------------- refusals and the interface
def test_refused_keyword_combinations_raise(monkeypatch):
    from unimedvl_amd import beam
    on = dict(do_sample=True, sampling=object(), draft_len=2, forced_ids=[[1]], top_logprobs=3, return_logits=True, constraint=object(),
              choices=["yes", "no"], repetition_penalty=1.2, presence_penalty=0.5, frequency_penalty=0.5, logit_bias={3: -1.0},
              no_repeat_ngram_size=3, top_k=5, top_p=0.9, min_p=0.1)
    assert set(on) == set(beam.BEAM_EXCLUDES)
    for k, v in on.items():
        with pytest.raises(ValueError, match=k):
            beam.check_beam_keywords(3, **{k: v})
        beam.check_beam_keywords(1, **{k: v})             # one beam: nothing to refuse
        beam.check_beam_keywords(3, **{k: beam.BEAM_EXCLUDES[k]})
    beam.check_beam_keywords(3, no_repeat_ngram_size=[0, 0], logit_bias={})
    with pytest.raises(ValueError, match="no_repeat_ngram_size"):
        beam.check_beam_keywords(3, no_repeat_ngram_size=[0, 2])
    monkeypatch.setenv("UMV_DECODE_FUSED_ARGMAX", "0")
    with pytest.raises(ValueError, match="UMV_DECODE_FUSED_ARGMAX"):
        beam.check_beam_keywords(2)
    monkeypatch.delenv("UMV_DECODE_FUSED_ARGMAX")
    for bad in (0, 11, 2.5, True):
        with pytest.raises(ValueError, match="num_beams"):
            ops.check_beams(bad)
    with pytest.raises(ValueError, match="vocabulary"):
        ops.check_beams(4, vocab=8)
    with pytest.raises(ValueError, match="64 rows"):
        ops.check_beams(4, vocab=100, rows=17)
    assert ops.check_beams(4, vocab=9, rows=16) == 4
    for bad in (dict(early_stopping="never"), dict(length_penalty=float("nan")), dict(num_return_sequences=4), dict(num_return_sequences=0)):
        with pytest.raises(ValueError):
            beam.check_beam_options(3, **{**dict(length_penalty=1.0, early_stopping=False, num_return_sequences=1), **bad})


def test_session_refuses_before_any_launch():
    from unimedvl_amd.beam import BeamDecodeSession

    class LLM:
        device = "cpu"
        cfg = type("Cfg", (), dict(vocab=330))
    naive = NaiveCache(2)
    naive.lens = [5]
    with pytest.raises(ValueError, match="PagedCache"):
        BeamDecodeSession(LLM(), naive, torch.tensor([1]), torch.tensor([5]), 4, 3)
    with pytest.raises(ValueError, match="do_sample"):
        BeamDecodeSession(LLM(), naive, torch.tensor([1]), torch.tensor([5]), 4, 3, do_sample=True)
    c = _prompt_cache([10] * 9)
    with pytest.raises(ValueError, match="64 rows"):
        BeamDecodeSession(LLM(), c, torch.zeros(9), torch.zeros(9), 4, 8)
    small = type("LLM", (), dict(device="cpu", cfg=type("Cfg", (), dict(vocab=6))))()
    with pytest.raises(ValueError, match="vocabulary"):
        BeamDecodeSession(small, c, torch.zeros(9), torch.zeros(9), 4, 3)
    assert c.pages_in_use() == 9


def test_the_public_interface_carries_the_keywords():
    from unimedvl_amd import _lib, bagel, build
    from unimedvl_amd import interactive_vqa_inferencer as vqa
    for fn in (bagel.Bagel.generate_text, bagel.Bagel.chat):
        sig = inspect.signature(fn).parameters
        assert [sig[k].default for k in ("num_beams", "length_penalty", "early_stopping", "num_return_sequences")] == [1, 1.0, False, 1]
        assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("num_beams", "length_penalty", "early_stopping", "num_return_sequences"))
    assert [vqa.DEFAULT_CONFIG[k] for k in ("num_beams", "length_penalty", "early_stopping", "num_return_sequences")] == [1, 1.0, False, 1]
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "unimedvl_hip.h")).read(), flags=re.S)
    for name in ("umv_beam_candidates", "umv_beam_step_end", "umv_beam_kv_copy"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr) and name in _lib._SIGS, name
    assert int(re.search(r"#define UMV_BEAM_K_MAX (\d+)", hdr).group(1)) == _lib.BEAM_K_MAX
    assert int(re.search(r"#define UMV_BEAM_TABLE_ENTRIES (\d+)", hdr).group(1)) == _lib.BEAM_TABLE_ENTRIES
    assert 2 * _lib.BEAM_K_MAX <= _lib.TOP_LOGPROBS_MAX
    assert build.LAST_SOURCES[-1] == "beam.hip" and os.path.exists(os.path.join(build.CSRC, "beam.hip"))
    # the ctypes mirror against the C struct's field list (every field a pointer or an int32, in the header's order)
    body = re.search(r"typedef struct \{([^}]*)\} umv_beam_step_args;", hdr).group(1)
    names = [n for decl in body.split(";") for n in re.findall(r"\*?\s*(\w+)\s*(?:,|$)", decl.split("*")[-1] if "*" in decl else decl.split(None, 1)[-1] if decl.strip() else "")]
    assert names == [f[0] for f in _lib.BeamStepArgs._fields_], names
    assert ctypes.sizeof(_lib.BeamStepArgs) == 19 * 8 + 7 * 4 + 4
