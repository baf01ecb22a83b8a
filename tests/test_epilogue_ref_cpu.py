"""The reference model of the GEMM epilogues (tests/epilogue_ref.py) itself, held to torch on the CPU over every bf16 value, and
the evidence that its acceptance rule for the activations (check_act) is sharp.  tests/test_gemm_epilogue_values_gpu.py compares the
kernels with this model."""
import torch
import torch.nn.functional as F

import epilogue_ref as E

BF16, F64 = E.BF16, E.F64
X = E.all_bf16()
FIN = torch.isfinite(X.to(F64))


def _pairs():
    """the operand pairs of the GPU tests' add chains: (all patterns scaled by the rows' powers of two, bias permutation) and
    (bf16 pre-activation, residual permutation)"""
    bias, res = E.patterns(E.BIAS_MULT, E.BIAS_OFFSET), E.patterns(E.RES_MULT, E.RES_OFFSET)
    for s in (1.0, 2.0, 0.5):
        acc = E.accumulate(s, X)
        yield acc.to(torch.float32), bias
        yield acc.to(torch.float32), res
        yield E.epilogue(acc, bias)[0].float(), res
    yield torch.zeros(65536), X                      # the bias-injected route: 0 + b


def test_add_chains_equal_torch_fp32():
    for a32, b in _pairs():
        want = (a32 + b.float()).to(BF16)
        got = E.rbf(E.add32(a32.to(F64), b)).to(BF16)
        assert E.count_diff(got, want) == 0
        assert E.count_diff(E.add32(a32.to(F64), b).to(torch.float32), a32 + b.float()) == 0
    # whole chains through epilogue()
    bias, res = E.patterns(E.BIAS_MULT, E.BIAS_OFFSET), E.patterns(E.RES_MULT, E.RES_OFFSET)
    acc = E.accumulate(1.0, X)
    out, pre = E.epilogue(acc, bias, None, res)
    want_pre = (acc.float() + bias.float()).to(BF16)
    assert E.count_diff(pre, want_pre) == 0
    assert E.count_diff(out, (want_pre.float() + res.float()).to(BF16)) == 0
    assert E.count_diff(E.epilogue(acc, None, None, res)[0], (acc.float().to(BF16).float() + res.float()).to(BF16)) == 0
    # -0 never arrives through an accumulator that starts at +0
    assert int((E.bits(E.epilogue(E.accumulate(1.0, X))[0]).to(torch.int32) & 0xFFFF == 0x8000).sum()) == 0


def test_operand_pairs_contain_ties_cancellations_and_carries():
    """the permutations are there so that the add steps meet their hard cases: count them"""
    def stats(a, b):
        a64, b64 = a.to(F64), b.to(F64)
        ok = torch.isfinite(a64) & torch.isfinite(b64)
        s = a64 + b64
        r = E.rbf(s)
        big = torch.maximum(a64.abs(), b64.abs())
        fin = ok & torch.isfinite(r)
        return {"ties": int((fin & ((s - r).abs() == 0.5 * E.bf16_ulp(s))).sum()),
                "cancel": int((ok & (s == 0) & (a64 != 0)).sum()),
                "carry": int((fin & (big > 0) & (torch.frexp(r.abs())[1] > torch.frexp(big)[1])).sum()),
                "lower": int((fin & (r != 0) & (torch.frexp(r.abs())[1] < torch.frexp(big)[1])).sum()),
                "overflow": int((ok & torch.isinf(r)).sum())}
    sb = stats(X, E.patterns(E.BIAS_MULT, E.BIAS_OFFSET))
    sr = stats(X, E.patterns(E.RES_MULT, E.RES_OFFSET))
    print("bias pairs", sb, "residual pairs", sr)
    assert sb["ties"] >= 200 and sb["cancel"] >= 200 and sb["carry"] >= 500 and sb["lower"] >= 200 and sb["overflow"] >= 1
    assert sr["ties"] >= 500 and sr["carry"] >= 100 and sr["lower"] >= 500


def _against_torch(kind, torch_fn, lo):
    """the ideal function against torch's own bf16 evaluation (fp32 inside) for x > lo; below, torch's fp32 evaluation saturates
    (SiLU: exp(-x) overflows at x <= -89 and the result is -0 where the value is still a bf16 subnormal) or cancels
    (GELU: 1 + tanh(u) in fp32 loses its bits from x = -4.5 down and is exactly 0 from about -5.5)"""
    t = torch_fn(X)
    want = E.rbf(E.IDEAL[kind](X)).to(BF16)
    st = E.steps(t, want)
    x64 = X.to(F64)
    differ, far = FIN & (st != 0), FIN & (st > 1)
    sel = FIN & (x64 > lo)
    print(kind, "differing", int(differ.sum()), "more than one step", int(far.sum()), "in", float(x64[differ].min()), float(x64[differ].max()))
    assert int((far & sel).sum()) == 0
    assert 1.0 - int((differ & sel).sum()) / int(sel.sum()) >= 0.999
    # non-finite inputs: the classes of the ideal function are torch's
    nf = ~FIN
    assert torch.equal(E.value_class(t[nf]), E.value_class(want[nf]))
    return int(differ.sum()), int(far.sum()), float(x64[far].min()), float(x64[far].max())


def test_silu_ideal_against_torch():
    differ, far, lo, hi = _against_torch("silu", F.silu, -87.0)
    assert (differ, far) == (17, 15) and -96.0 <= lo and hi <= -89.0        # all of torch's misses lie in its saturated tail


def test_gelu_ideal_against_torch():
    differ, far, lo, hi = _against_torch("gelu_tanh", lambda v: F.gelu(v, approximate="tanh"), -4.5)
    assert (differ, far) == (155, 145) and -10.25 <= lo and hi <= -4.5625


def test_textbook_gelu_cancels_in_fp64():
    """why gelu_ideal is not 0.5 x (1 + tanh u)"""
    import math
    x = X.to(F64)
    u = math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)
    textbook = 0.5 * x * (1.0 + torch.tanh(u))
    lost = FIN & (textbook == 0) & (E.rbf(E.gelu_ideal(X)) != 0)
    print("textbook form exactly 0 where the value is a nonzero bf16 number:", int(lost.sum()))
    assert int(lost.sum()) >= 50


def test_nonfinite_classes_of_the_ideal_functions():
    for kind in ("silu", "gelu_tanh"):
        got = E.rbf(E.IDEAL[kind](torch.tensor([float("inf"), float("-inf"), float("nan")], dtype=BF16)))
        assert E.value_class(got).tolist() == [2, 4, 4]        # +inf -> +inf, -inf -> NaN (x * 0), NaN -> NaN


def test_check_act_rejects_the_clamped_formula_and_accepts_the_unclamped():
    """x * rcp(1 + exp2(min(t, 126))), the form the epilogues had, returns x * 2^-126 in the left tail: check_act must refuse it -
    and must accept the same formula without the clamp, whose tail flushes to -0."""
    import pytest
    for kind, formula, n_bad in (("silu", E.silu_formula, 15569), ("gelu_tanh", E.gelu_formula, 15967)):
        r = E.act_report(formula(X, True), X, kind)
        assert r["violations"] == n_bad and r["differ"] == 0
        with pytest.raises(AssertionError):
            E.check_act(formula(X, True), X, kind)
        r = E.check_act(formula(X, False), X, kind)
        assert r["violations"] == 0 and r["equal_share"] == 1.0
        # the two forms agree bit for bit outside the flush band
        ideal = E.IDEAL[kind](X)
        band = FIN & (ideal.abs() < E.FLUSH * X.to(F64).abs().clamp_min(1.0))
        same = E.canon_bits(formula(X, True)) == E.canon_bits(formula(X, False))
        assert bool(same[FIN & ~band].all())
    # the rule is sharp in the other direction too: a result two values off, or a flushed result of the wrong sign, is refused
    good = E.rbf(E.silu_ideal(X)).to(BF16)
    off = (E.bits(good).to(torch.int32) + 2).to(torch.int16).view(BF16)
    assert E.act_report(torch.where((X.to(F64) > 1) & (X.to(F64) < 2), off, good), X, "silu")["violations"] == 127
    wrong_sign = torch.where(X.to(F64) < -200, torch.full_like(good, 2.0 ** -130), good)
    assert E.act_report(wrong_sign, X, "silu")["violations"] > 0
