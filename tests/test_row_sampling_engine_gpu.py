"""Per-request sampling parameters through the engine at the tiny configuration: DecodeSession(row_sampling=...) against the scalar
session, graph replay against the un-captured step, set_slot(sampling=...) without a re-capture, and the batcher's per-request mode - a
request's tokens and log-probabilities must not depend on its slot, its neighbours, the admission order or check_every.  Everything is
exact.  Wherever two runs are compared the attention key split is pinned: bit identity across sessions holds at equal nsplit."""
import pytest
import torch

from conftest import NEW_TOKEN_IDS

pytestmark = pytest.mark.gpu
T = 0.7
SEED = 77
PROMPTS = [[11, 22, 33, 44, 55], [66, 77, 88], [99, 111, 122, 133]]
STEPS = 8


@pytest.fixture(scope="module")
def model(tiny_weights):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from unimedvl_amd.bagel import Bagel
    from unimedvl_amd.config import UniMedVLConfig
    cfg, sd, _, _ = tiny_weights
    return Bagel(UniMedVLConfig.from_dict(cfg), lambda n: sd[n], device="cuda", visual_gen=False)


@pytest.fixture(autouse=True)
def pinned_split(monkeypatch):
    monkeypatch.setenv("UMV_DECODE_NSPLIT", "2")


def _params(**kw):
    from unimedvl_amd.sampling import SamplingParams
    return SamplingParams(**kw)


def _session(model, steps=STEPS, B=3, **kw):
    from unimedvl_amd.decode import DecodeSession
    from unimedvl_amd.kvcache import NaiveCache

    class Tok:
        def encode(self, s):
            return PROMPTS[int(s) % 3] + [int(s) // 3 + 5] * (int(s) // 3 > 0)
    cache = NaiveCache(model.cfg.layers)
    gi, kvl, rope = model.prepare_prompts([0] * B, [0] * B, [str(i) for i in range(B)], Tok(), NEW_TOKEN_IDS)
    cache = model.forward_cache_update_text(cache, **gi)
    gi = model.prepare_start_tokens(kvl, rope, NEW_TOKEN_IDS)
    with torch.no_grad():
        return DecodeSession(model.language_model, cache, gi["packed_start_tokens"], gi["packed_query_position_ids"], steps, **kw)


def _run(model, steps=STEPS, **kw):
    s = _session(model, steps, **kw)
    with torch.no_grad():
        s.step(steps)
    torch.cuda.synchronize()
    return s


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ----------------------------------------------------------------------------- 6. the session
SCALAR = {
    "greedy": dict(),
    "sampled": dict(do_sample=True, temperature=T),
    "truncated": dict(do_sample=True, temperature=T, top_k=20, top_p=0.9),
    "penalised": dict(do_sample=True, temperature=T, min_p=0.05, repetition_penalty=1.2, presence_penalty=0.5, frequency_penalty=0.25),
}


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("name", list(SCALAR))
def test_uniform_rows_equal_the_scalar_session(model, name, use_graph):
    kw = SCALAR[name]
    ctx = [p + [NEW_TOKEN_IDS["bos_token_id"]] for p in PROMPTS]
    want = _run(model, use_graph=use_graph, seed=SEED, logprobs=True, penalty_context_ids=ctx, **kw)
    got = _run(model, use_graph=use_graph, seed=SEED, logprobs=True, penalty_context_ids=ctx, row_sampling=[_params(**kw)] * 3,
               row_streams=[0, 1, 2])
    assert got.step_end == "rows" and (got.graph is not None) == use_graph
    assert torch.equal(want.pred_ids, got.pred_ids) and torch.equal(want.in_ids, got.in_ids), f"{name}: tokens"
    assert _same_bits(want.pred_logprobs, got.pred_logprobs), f"{name}: log-probabilities"
    if want.truncated:
        assert _same_bits(want.pred_cut_y, got.pred_cut_y) and torch.equal(want.pred_n_kept, got.pred_n_kept), f"{name}: cutoffs"
    else:
        assert (got.pred_cut_y == float("-inf")).all() and (got.pred_n_kept == model.cfg.vocab).all()
    assert got.row_table[:, 1].tolist() == [STEPS] * 3, "every row drew once per step"
    assert (got.pen is not None) == (name == "penalised")


def _mixed():
    return [_params(), _params(do_sample=True, temperature=T, top_p=0.8, seed=5),
            _params(do_sample=True, temperature=1.2, repetition_penalty=1.3, frequency_penalty=0.2)]


def test_mixed_session_graph_replay_equals_eager(model):
    g = _run(model, use_graph=True, seed=SEED, logprobs=True, row_sampling=_mixed())
    e = _run(model, use_graph=False, seed=SEED, logprobs=True, row_sampling=_mixed())
    assert g.graph is not None and e.graph is None
    assert torch.equal(g.pred_ids, e.pred_ids) and _same_bits(g.pred_logprobs, e.pred_logprobs)
    assert _same_bits(g.pred_cut_y, e.pred_cut_y) and torch.equal(g.pred_n_kept, e.pred_n_kept) and torch.equal(g.row_table, e.row_table)
    # row 0 is the greedy session's sample 0, whatever its neighbours do
    greedy = _run(model, use_graph=True, logprobs=True)
    assert torch.equal(g.pred_ids[:, 0], greedy.pred_ids[:, 0]) and _same_bits(g.pred_logprobs[:, 0].contiguous(), greedy.pred_logprobs[:, 0].contiguous())
    assert (g.pred_n_kept[:, 0] == model.cfg.vocab).all() and (g.pred_n_kept[:, 1] < model.cfg.vocab).any()


# ----------------------------------------------------------------------------- 7. set_slot
def test_set_slot_changes_a_slot_without_a_recapture(model):
    half = STEPS // 2

    def run(change):
        s = _session(model, use_graph=True, seed=SEED, logprobs=True, row_sampling=_mixed(), row_penalties=True)
        graph = s.graph
        with torch.no_grad():
            s.step(half)
            if change:
                torch.cuda.synchronize()
                tok, kv, pos = int(s.ids[1]), int(s.kv_len[1]) - 1, int(s.tok_pos[1])
                s.set_slot(1, tok, kv, pos, sampling=_params(), stream=1, draw=0)          # slot 1 goes on greedy
                assert s.row_table[1].tolist()[1] == 0 and s.row_params[1] == _params()
            s.step(half)
        torch.cuda.synchronize()
        assert s.graph is graph, "no re-capture"
        return s
    base, changed = run(False), run(True)
    for b in (0, 2):        # the untouched slots: bit-identical to the run without the call
        assert torch.equal(base.pred_ids[:, b], changed.pred_ids[:, b])
        assert _same_bits(base.pred_logprobs[:, b].contiguous(), changed.pred_logprobs[:, b].contiguous())
        assert torch.equal(base.pred_n_kept[:, b], changed.pred_n_kept[:, b])
    assert torch.equal(base.pred_ids[:half], changed.pred_ids[:half])
    # slot 1: truncated before the call, greedy after it
    assert (changed.pred_n_kept[half:, 1] == model.cfg.vocab).all() and (changed.pred_cut_y[half:, 1] == float("-inf")).all()
    assert (base.pred_n_kept[:, 1] < model.cfg.vocab).any()
    assert changed.row_table[:, 1].tolist() == [STEPS, half, STEPS]
    with pytest.raises(ValueError, match="row_sampling"):
        _session(model, use_graph=False).set_slot(0, 5, 3, 3, sampling=_params())
    plain = _session(model, use_graph=False, row_sampling=[_params()] * 3)
    with pytest.raises(ValueError, match="row_penalties"):
        plain.set_slot(0, 5, 3, 3, sampling=_params(presence_penalty=0.5))


def test_rewind_leaves_the_draw_counters(model):
    s = _session(model, 8, use_graph=True, seed=SEED, row_sampling=[_params(do_sample=True, temperature=T)] * 3)
    with torch.no_grad():
        s.step(4)
        first = s.pred_ids[:4].clone()
        s.rewind_outputs()
        s.step(4)
    assert s.row_table[:, 1].tolist() == [8, 8, 8] and (s.step_idx == 4).all()
    # the scalar session's second round repeats the noise of its first (keyed by the round-local step); this one's does not: its
    # eight draws are those of one eight-step round
    whole = _run(model, 8, use_graph=True, seed=SEED, row_sampling=[_params(do_sample=True, temperature=T)] * 3)
    assert torch.equal(torch.cat([first, s.pred_ids[:4]]), whole.pred_ids)


# ----------------------------------------------------------------------------- 8. the batcher
def _requests():
    g = torch.Generator().manual_seed(21)
    reqs = [([torch.randn(3, 42, 56, generator=g).clamp(-1, 1)] if i % 2 == 0 else [], f"{5 + i} {17 + 3 * i} {40 + i} {17 + 3 * i}")
            for i in range(7)]
    pars = [_params(), _params(do_sample=True, temperature=T, seed=101), _params(do_sample=True, top_k=1, seed=102),
            _params(repetition_penalty=1.3, presence_penalty=0.4), _params(do_sample=True, temperature=1.1, top_p=0.85, min_p=0.02, seed=104),
            _params(), _params(do_sample=True, temperature=T, frequency_penalty=0.3, repetition_penalty=1.2, seed=106)]
    return reqs, pars


def _serve(model, order, check_every, slots=3):
    from oracle.toy_tokenizer import ToyTokenizer
    from unimedvl_amd.serving import ContinuousBatcher
    reqs, pars = _requests()
    srv = ContinuousBatcher(model, ToyTokenizer(NEW_TOKEN_IDS), NEW_TOKEN_IDS, lambda x: x, slots=slots, max_context=256, max_new_tokens=7,
                            check_every=check_every, logprobs=True, penalize_prompt=True, per_request_sampling=True, seed=9)
    rids = {i: srv.submit(*reqs[i], sampling=pars[i]) for i in order}
    got = srv.run()
    return {i: (got[r], srv.logprobs[r]) for i, r in rids.items()}


def test_batcher_requests_do_not_depend_on_slot_order_or_round_length(model):
    from oracle.toy_tokenizer import ToyTokenizer
    reqs, pars = _requests()
    base = _serve(model, range(7), 3)
    for what, other in (("reversed", _serve(model, reversed(range(7)), 3)), ("check_every 16", _serve(model, range(7), 16))):
        for i in range(7):
            assert other[i][0] == base[i][0], f"{what}: request {i} answers {other[i][0]!r}, not {base[i][0]!r}"
            assert other[i][1] == base[i][1], f"{what}: request {i}: log-probabilities differ"
    for i in range(7):
        alone = _serve(model, [i], 3)
        assert alone[i] == base[i], f"request {i} served alone: {alone[i]} against {base[i]}"
    tok = ToyTokenizer(NEW_TOKEN_IDS)
    for i in (0, 5, 2):      # the greedy requests, and top_k = 1 (greedy unless a step's maximum is tied)
        want = model.chat(tok, NEW_TOKEN_IDS, lambda x: x, reqs[i][0], reqs[i][1], max_length=8)
        assert base[i][0] == want, f"request {i}: {base[i][0]!r} against chat's greedy {want!r}"
    assert all(len(lp) > 0 for _, lp in base.values())


def test_batcher_defaults_and_refusals(model):
    from oracle.toy_tokenizer import ToyTokenizer
    from unimedvl_amd.serving import ContinuousBatcher
    tok = ToyTokenizer(NEW_TOKEN_IDS)
    mk = lambda **kw: ContinuousBatcher(model, tok, NEW_TOKEN_IDS, lambda x: x, slots=3, max_context=256, max_new_tokens=6, **kw)   # noqa: E731
    with pytest.raises(ValueError, match="per_request_sampling"):
        mk().submit(None, "5 6 7", sampling=_params())
    with pytest.raises(ValueError, match="per_request_sampling"):
        mk(seed=3)
    with pytest.raises(ValueError, match="64 slots"):
        ContinuousBatcher(model, tok, NEW_TOKEN_IDS, lambda x: x, slots=65, per_request_sampling=True)
    # a request that gives no parameters takes the batcher-wide ones: here greedy, the plain batcher's answers
    a, b = mk(per_request_sampling=True, seed=1), mk()
    ra, rb = [a.submit(None, f"{7 + i} 9 11") for i in range(4)], [b.submit(None, f"{7 + i} 9 11") for i in range(4)]
    ga, gb = a.run(), b.run()
    assert [ga[r] for r in ra] == [gb[r] for r in rb]


# ----------------------------------------------------------------------------- 9. nothing changes without the mode
def test_a_session_without_the_mode_is_todays(model):
    for kw, end, keys in ((dict(), "argmax", {"argmax_partial", "sample"}),
                          (dict(do_sample=True, temperature=T, seed=SEED), "argmax", {"argmax_partial", "sample"}),
                          (dict(logprobs=True), "logprob", {"argmax_partial", "lse_partial", "sample"}),
                          (dict(do_sample=True, temperature=T, top_k=5), "truncated", {"argmax_partial", "lse_partial", "sample"})):
        s = _session(model, 4, use_graph=False, **kw)
        assert s.step_end == end and set(s.lm_head_kw) == keys, (kw, s.step_end, set(s.lm_head_kw))
        assert s.row_table is None and s.row_params is None and s.pen is None and s.pen_count is None and s.pen_list is None
    with pytest.raises(ValueError, match="64 samples"):
        _session(model, 2, B=65, use_graph=False, row_sampling=[_params()] * 65)
