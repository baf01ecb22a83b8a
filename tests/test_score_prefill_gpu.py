"""Bagel.score_prefill - the prefill-time scorer - through the engine at the tiny configuration, against the CPU oracle run
teacher-forced over the same rows (OracleBagel.llm_forward + lm_head, then an fp64 log-softmax).

The bound: a log-probability is a logit minus a log-sum-exp of logits, so it moves at most twice the largest logit error: 0.5 = 2 x
the project's 0.25 logit bound.  `score` - the forced decode session - is held to the same assertion as the yardstick.

Such a bound sees a layout bug only if the model is sensitive to the layout, and the tiny random model is not: unit q / k gains give
near-uniform attention, and at rope_theta = 1e6 one position step turns a handful of the 128 head dimensions.  So the model of this
module is the tiny one with - in copies of the configuration and the state dict - rope_theta = 10, q_norm gains x 3 and k_norm gains
x 2 (the peaked-attention test's), the lm_head weight x 7.25, behind a context of a 64-patch image and a 24-token prompt; chosen on
the CPU so that THE ORACLE ALONE meets the conditions the mixed-set test asserts first (`_sensitive`): its per-token values span
more than 5, and both scoring row i against t_{i+1} and moving every rope position by one move more than 90 % of the tokens by more
than 1.0.  The oracle runs its 'flash' attention model (P rounded to bf16, as the kernels hold it; the peaked-attention test's
reference): with these gains its own two attention models are 0.7 apart in these values.

The margins are thin on both sides, and that is a property of the numbers, not of the scorer: a layout error has to move a value by
more than 1.0 and the arithmetic may move it by 0.5, while the values reach -37, where neighbouring bf16 logits are 0.125 - 0.25
apart.  On an MI355X (profiles/score_prefill_tests.txt): oracle span 37.4, targets shifted 55 of 58 tokens (50 of 54 without the end
token), positions off by one 53 of 58 (51 of 54); largest difference from the oracle 0.470 for score_prefill and 0.487 for `score`
itself.  At lm_head x 7.0 the position condition fails (52 of 58), at x 7.5 `score` misses the bound (0.506) - so does every larger
scale, for both scorers alike (x 12: 0.81 and 0.77).  The fp8-weight case needs no layout sensitivity (the layout code is shared) and
runs on the tiny weights as they are, as the fp8 engine tests do.
"""
import math

import pytest
import torch

from conftest import NEW_TOKEN_IDS

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
BOUND = 0.5
BOS, EOS = NEW_TOKEN_IDS["bos_token_id"], NEW_TOKEN_IDS["eos_token_id"]
LM_HEAD_SCALE, Q_GAIN, K_GAIN, ROPE_THETA = 7.25, 3.0, 2.0, 10.0
ORACLE_ATTN = "flash"       # the oracle's attention model: P rounded to bf16 as the kernels hold it ("sdpa": an exact fp32 softmax)
PROMPT = torch.randint(5, 290, (24,), generator=torch.Generator().manual_seed(3)).tolist()
LONG40 = torch.randint(5, 290, (40,), generator=torch.Generator().manual_seed(40)).tolist()
ident = lambda x: x   # noqa: E731


class Tok:
    """strings are space-separated token ids"""

    def encode(self, s):
        return [int(v) for v in s.split()]

    def decode(self, ids):
        return "".join({BOS: "<|im_start|>", EOS: "<|im_end|>"}.get(int(i), f" {int(i)}") for i in ids)


def _sensitive_weights(cfg, sd):
    cfg = dict(cfg, rope_theta=ROPE_THETA)
    sd = dict(sd)
    for k, v in list(sd.items()):
        gain = Q_GAIN if k.endswith("q_norm.weight") else K_GAIN if k.endswith("k_norm.weight") else LM_HEAD_SCALE if k == "language_model.lm_head.weight" else None
        if gain is not None:
            sd[k] = (v.float() * gain).to(BF16)
    return cfg, sd


class Setup:
    def __init__(self, tiny_weights, weight_dtype="bf16", sensitive=True):
        if not torch.cuda.is_available():
            pytest.fail("GPU tests need a GPU")
        from oracle import fp8
        from oracle.unimedvl_cpu import KVCache, OracleBagel
        from unimedvl_amd.bagel import Bagel
        from unimedvl_amd.config import UniMedVLConfig
        cfg, sd, vae_sd, _ = tiny_weights
        if sensitive:
            cfg, sd = _sensitive_weights(cfg, sd)
        c = UniMedVLConfig.from_dict(cfg)
        assert c.rope_theta == cfg["rope_theta"]
        c.llm_weight_dtype = weight_dtype
        self.model = Bagel(c, lambda n: sd[n], device="cuda", visual_gen=False)
        self.img = torch.randn(3, 112, 112, generator=torch.Generator().manual_seed(2)).clamp(-1, 1)
        self.prompt = " ".join(str(t) for t in PROMPT)
        # the oracle's context, prefilled once (fp8 weights: the oracle runs on the dequantised weights, as the fp8 engine tests calibrate)
        self.oracle = o = OracleBagel(cfg, fp8.dequantised_weights(sd) if weight_dtype == "fp8" else sd, vae_sd, attn_impl=ORACLE_ATTN)
        self.oc = KVCache(cfg["layers"], 1)
        kv, rope = o.update_vit(self.oc, [0], [0], [self.img], NEW_TOKEN_IDS)
        self.kv, self.rope = o.update_text(self.oc, kv, rope, [[BOS] + PROMPT + [EOS]])

    def score_prefill(self, cands, **kw):
        return self.model.score_prefill(Tok(), NEW_TOKEN_IDS, ident, [self.img], self.prompt, cands, **kw)

    def score(self, cands, **kw):
        return self.model.score(Tok(), NEW_TOKEN_IDS, ident, [self.img], self.prompt, cands, **kw)

    def oracle_values(self, toks, dpos=0, shift=0):
        """per candidate the fp64 log-probabilities of its tokens, teacher-forced: rows [bos, t_0, ..] at the positions behind the context
        (+ dpos), row i scored against t_{i + shift} (cyclically)"""
        o, out = self.oracle, []
        for t in toks:
            pos = torch.arange(self.rope[0] + dpos, self.rope[0] + dpos + len(t))
            h = o.llm_forward(o.embed(torch.tensor([BOS] + t[:-1])), [len(t)], pos, self.oc.clone(), True, True, "und")
            lp = torch.log_softmax(o.lm_head(h).double(), -1)
            out.append(lp[torch.arange(len(t)), torch.tensor(t[shift:] + t[:shift])])
        return out


@pytest.fixture(scope="module")
def setup(tiny_weights):
    return Setup(tiny_weights)


def _sensitive(s, toks):
    """the conditions of the module docstring, on the oracle alone -> its values"""
    want = s.oracle_values(toks)
    flat = torch.cat(want)
    span = float(flat.max() - flat.min())
    moved = [float(((torch.cat(s.oracle_values(toks, **kw)) - flat).abs() > 1.0).float().mean()) for kw in (dict(shift=1), dict(dpos=1))]
    print(f"oracle alone, {len(flat)} tokens: values span {span:.1f}; targets shifted by one row move {moved[0]:.1%} of them by more than 1, "
          f"rope positions off by one {moved[1]:.1%}")
    assert span > 5 and moved[0] > 0.9 and moved[1] > 0.9, (span, moved)
    return want


def _worst(res, want):
    return max(float((torch.tensor(r["token_logprobs"], dtype=torch.float64) - w).abs().max()) for r, w in zip(res, want))


def _own_answer(s):
    answer, own, _ = s.model.chat(Tok(), NEW_TOKEN_IDS, ident, [s.img], s.prompt, max_length=6, return_logprobs=True)
    assert len(own) >= 1
    return own


# ----------------------------------------------------------------------------- 1. a mixed set
@pytest.mark.parametrize("append_eos", [True, False])
def test_mixed_set_against_the_oracle(setup, append_eos):
    s = setup
    cands = [_own_answer(s), [7, 8], [9, 10, 11, 12, 13, 14, 15], LONG40]
    toks = [list(c) + ([EOS] if append_eos else []) for c in cands]
    want = _sensitive(s, toks)
    got, forced = s.score_prefill(cands, append_eos=append_eos), s.score(cands, append_eos=append_eos)
    assert s.model.language_model.last_token_logprobs["fused"] is True
    assert [r["token_ids"] for r in got] == toks == [r["token_ids"] for r in forced]
    for r in got:
        assert len(r["token_logprobs"]) == len(r["token_ids"]) and all(math.isfinite(v) and v <= 0 for v in r["token_logprobs"])
        assert r["logprob"] == float(torch.tensor(r["token_logprobs"], dtype=torch.float64).sum())
    worst_p, worst_s = _worst(got, want), _worst(forced, want)
    print(f"append_eos={append_eos}: largest |token logprob - oracle|: score_prefill {worst_p:.4f}, score {worst_s:.4f} (bound {BOUND})")
    assert worst_s <= BOUND, f"score (the yardstick) is {worst_s} from the oracle"
    assert worst_p <= BOUND, f"score_prefill is {worst_p} from the oracle"
    totals = sorted((float(w.sum()) for w in want), reverse=True)
    if totals[0] - totals[1] > 1.0:
        best = lambda res: max(range(len(res)), key=lambda i: res[i]["logprob"])   # noqa: E731
        assert best(got) == best(forced)


# ----------------------------------------------------------------------------- 2. both sides of the 64-row edge
EDGE = [[9, 10, 11, 12, 13, 14, 15], LONG40, list(range(100, 114))]          # + the end token each: 8 + 41 + 15 = 64 rows


@pytest.mark.parametrize("extra", [0, 1])
def test_both_sides_of_the_64_row_edge(setup, extra):
    s = setup
    cands = EDGE[:2] + [EDGE[2] + [77] * extra]
    toks = [c + [EOS] for c in cands]
    assert sum(len(t) for t in toks) == 64 + extra
    want = s.oracle_values(toks)
    got = s.score_prefill(cands)
    worst = _worst(got, want)
    print(f"{64 + extra} rows: largest |token logprob - oracle| {worst:.4f}")
    assert [r["token_ids"] for r in got] == toks and worst <= BOUND


# ----------------------------------------------------------------------------- 3 / 4. repeatability, chunking, one forward pass
def test_repeatable_and_independent_of_the_chunking(setup, monkeypatch):
    s = setup
    lm = s.model.language_model
    cands = EDGE[:2] + [EDGE[2] + [77]]
    calls = []
    plain = lm.forward_inference
    monkeypatch.setattr(lm, "forward_inference", lambda *a, **kw: (calls.append(list(kw["query_lens"])), plain(*a, **kw))[1])
    first = s.score_prefill(cands)
    assert len(calls) == 3 and calls[-1] == [8, 41, 16], calls       # the image, the prompt, then ONE pass over the candidates' rows
    assert lm.last_token_logprobs["rows_per_pass"] == 65
    assert s.score_prefill(cands) == first
    chunked = s.score_prefill(cands, rows_per_pass=16)
    assert lm.last_token_logprobs["rows_per_pass"] == 16 and lm.last_token_logprobs["workspace_bytes"] == 16 * (20 * 8 + 4)
    assert chunked == first                                          # only the lm_head is chunked, and a row's bits do not depend on its chunk
    assert s.score_prefill(cands, rows_per_pass=1) == first
    with pytest.raises(ValueError, match="rows_per_pass"):
        s.score_prefill(cands, rows_per_pass=0)


# ----------------------------------------------------------------------------- 5. the fallback
def test_unfused_fallback(setup):
    """fused=False: ops.gemm into a logits chunk, then ops.token_logprob.  At 65 rows both arms run the MFMA tiles - the same stored logits
    - and differ by the order of the sums only: 1e-4 each from fp64, asserted at 2e-4.  At 64 rows and below ops.gemm takes the
    weight-streaming kernel, whose 8-wave split of K can round a logit to the neighbouring bf16 value (one ulp: up to 0.25 at these
    magnitudes): there the arm is held to the oracle, and the difference is printed."""
    s = setup
    lm = s.model.language_model
    cands = EDGE[:2] + [EDGE[2] + [77]]
    fused, plain = s.score_prefill(cands), s.score_prefill(cands, fused=False)
    assert lm.last_token_logprobs == {"fused": False, "rows_per_pass": 65, "workspace_bytes": 65 * 320 * 2}
    d = max(abs(a - b) for rf, rp in zip(fused, plain) for a, b in zip(rf["token_logprobs"], rp["token_logprobs"]))
    print(f"65 rows: largest |fused - unfused| {d:.3g}")
    assert [r["token_ids"] for r in fused] == [r["token_ids"] for r in plain] and d <= 2e-4
    assert s.score_prefill(cands, fused=False, rows_per_pass=1024) == plain
    want = s.oracle_values([c + [EOS] for c in EDGE])
    few, few_plain = s.score_prefill(EDGE), s.score_prefill(EDGE, fused=False)
    d = max(abs(a - b) for rf, rp in zip(few, few_plain) for a, b in zip(rf["token_logprobs"], rp["token_logprobs"]))
    print(f"64 rows (unfused arm on the weight-streaming GEMM): largest |fused - unfused| {d:.3g}, unfused vs oracle {_worst(few_plain, want):.4f}")
    assert _worst(few_plain, want) <= BOUND


# ----------------------------------------------------------------------------- 6 / 7. strings, errors
def test_strings_and_errors(setup, monkeypatch):
    s = setup
    cands = [[7, 8], [9, 10, 11, 12, 13, 14, 15]]
    res = s.score_prefill(cands)
    assert s.score_prefill([" ".join(str(t) for t in c) for c in cands]) == res
    bare = s.score_prefill(cands, append_eos=False)
    assert [r["token_ids"] for r in bare] == cands
    with pytest.raises(ValueError, match="64"):
        s.score_prefill([[7]] * 65)
    with pytest.raises(ValueError, match="64"):
        s.score_prefill([])
    with pytest.raises(ValueError, match="empty"):
        s.score_prefill([[7], []], append_eos=False)
    with pytest.raises(ValueError, match="vocab"):
        s.score_prefill([[7, s.model.cfg.vocab]])
    assert len(s.score_prefill([[7]] * 64)) == 64
    monkeypatch.setattr(s.model.cfg, "max_position", s.rope[0] + 3)          # the start token sits at s.rope[0]: three rows fit, four do not
    assert len(s.score_prefill([[7, 8]])) == 1
    with pytest.raises(ValueError, match="max_position"):
        s.score_prefill([[7, 8], [7, 8, 9]])


# ----------------------------------------------------------------------------- 8. the context cache
def test_context_cache_is_left_as_it_was(setup, monkeypatch):
    from unimedvl_amd.kvcache import NaiveCache
    s = setup
    seen = {}
    plain = NaiveCache.merged

    def merged(caches, *a, **kw):
        ctx = caches[0]
        assert all(c is ctx for c in caches)
        n = max(ctx.lens)
        seen.update(ctx=ctx, lens=list(ctx.lens), n=n, k=[sl.k[:, :, :n].clone() for sl in ctx.slabs], vt=[sl.vt[:, :, :, :n].clone() for sl in ctx.slabs],
                    ptr=[sl.k.data_ptr() for sl in ctx.slabs])
        return plain(caches, *a, **kw)
    monkeypatch.setattr(NaiveCache, "merged", staticmethod(merged))
    s.score_prefill([[7, 8], LONG40])
    ctx, n = seen["ctx"], seen["n"]
    assert ctx.lens == seen["lens"] == s.kv and [sl.k.data_ptr() for sl in ctx.slabs] == seen["ptr"]
    for sl, k, vt in zip(ctx.slabs, seen["k"], seen["vt"]):
        assert torch.equal(sl.k[:, :, :n], k) and torch.equal(sl.vt[:, :, :, :n], vt)


# ----------------------------------------------------------------------------- 9. the inferencer
def test_inferencer_score_prefill(setup):
    import numpy as np
    from PIL import Image
    from unimedvl_amd.interactive_vqa_inferencer import VQAInferencer
    from unimedvl_amd.transforms import ImageTransform
    s = setup
    pil = Image.fromarray(np.random.default_rng(3).integers(0, 255, (60, 84, 3), dtype=np.uint8))
    v = VQAInferencer({"max_new_tokens": 6, "do_sample": False})
    with pytest.raises(RuntimeError, match="load_model"):
        v.score_prefill(pil, "5 6 7 8", [[7]])
    v.load_model(model=s.model, tokenizer=Tok(), new_token_ids=NEW_TOKEN_IDS)
    v.image_transform = ImageTransform(56, 28, 14)
    cands = [[7, 8], "9 10 11", LONG40]
    for eos in (True, False):
        want = s.model.score_prefill(Tok(), NEW_TOKEN_IDS, ImageTransform(56, 28, 14), [pil], "5 6 7 8", cands, append_eos=eos)
        assert v.score_prefill(pil, "5 6 7 8", cands, append_eos=eos) == want
    assert [r["token_ids"] for r in want] == [[7, 8], [9, 10, 11], LONG40]


# ----------------------------------------------------------------------------- 10. an e4m3 lm_head takes the fallback
def test_fp8_weights_take_the_fallback(tiny_weights):
    s = Setup(tiny_weights, "fp8", sensitive=False)
    lm = s.model.language_model
    assert lm.w.lm_head.w8 is not None
    cands = [[7, 8], [9, 10, 11, 12, 13, 14, 15], LONG40, list(range(100, 114))]
    toks = [c + [EOS] for c in cands]
    want = s.oracle_values(toks)
    got = s.score_prefill(cands)
    assert lm.last_token_logprobs["fused"] is False and sum(len(t) for t in toks) == 67
    worst = _worst(got, want)
    print(f"fp8 weights, 67 rows: largest |token logprob - oracle on the dequantised weights| {worst:.4f}")
    assert [r["token_ids"] for r in got] == toks and worst <= BOUND
