"""Sampled speculative decode on the host (include/unimedvl_hip.h, "speculative decode with sampling"): the plain-Python model of the
commit launch (tests/spec_sample_ref.py) reproduces the plain per-row sequence t_i = f(t_<i, i) for ANY drafts, because row j of a
step picks with the draw counter of the token it would emit; m = 0 leaves the draws alone; the host noise model is the documented
stream; and the ctypes mirror of the new argument struct is the C struct as the host compiler lays it out."""
import ctypes
import math
import os
import random
import shutil
import subprocess

import pytest

import spec_sample_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "unimedvl_hip.h")
INCLUDE = os.path.join(ROOT, "include")
V = 97


def _pick(seq, draw):
    """a deterministic 'sampler': a token that depends on the whole prefix AND on the draw counter, with repeats (so lookups hit)"""
    h = R.splitmix64(sum((i + 1) * t for i, t in enumerate(seq)) * 31 + draw * 0x9E37)
    return seq[-3] if len(seq) >= 3 and h % 3 == 0 else h % 11


def _sample(k, limit, context, predicted=None, out_ld=40, hist_ld=None):
    hist = list(context) + [5]
    return R.Sample(k, 5, slot=len(context), pos=len(context), out_ld=out_ld, limit=limit, hist=hist,
                    hist_ld=hist_ld if hist_ld is not None else len(hist) + out_ld, vocab=V, ngram=(1, 3), predicted=predicted,
                    pred_len=0 if predicted is None else len(predicted))


@pytest.mark.parametrize("k", [1, 3, 7])
@pytest.mark.parametrize("drafts", ["lookup", "perfect", "empty", "random", "corrupted"])
def test_any_drafts_give_the_plain_sequence(k, drafts):
    rng = random.Random(k * 10 + len(drafts))
    context = [rng.randrange(11) for _ in range(20)]
    count = 33
    plain = R.plain_sampled(_pick, context, 5, count)
    assert plain != R.plain_sampled(lambda s, d: _pick(s, 0), context, 5, count), "the toy sampler must depend on the draw"
    predicted, redraft = None, None
    if drafts == "perfect":
        predicted = list(plain)
    elif drafts == "corrupted":
        predicted = [t if i % 5 != 3 else (t + 1) % 11 for i, t in enumerate(plain)]
    elif drafts == "random":
        def redraft(s):
            s.n_draft = rng.randrange(k + 1)
            s.ids[1:] = [rng.randrange(11) for _ in range(s.n_draft)] + [s.ids[0]] * (k - s.n_draft)
    s = _sample(k, count, [] if drafts == "empty" else context, predicted)
    if drafts == "empty":
        s.ngram = (30, 30)         # no suffix that long ever matches: no drafts at all
    s.draft()
    kv0, pos0 = s.kv_len, s.tok_pos[0]
    steps = R.run(s, _pick, context, redraft=redraft)
    assert s.out[:count] == plain and s.n_out == count
    assert s.draws == [count + j for j in range(k + 1)], "the draws end at n_out + j"
    # every step emits its accepted drafts plus one; only the last step can be clipped by the limit (accepted, not emitted)
    assert s.stats[0] == steps and count - steps <= s.stats[2] <= count - steps + k
    if drafts == "perfect":
        assert steps == math.ceil(count / (k + 1)) and s.stats[2] <= s.stats[1]
    if drafts == "empty":
        assert steps == count and s.stats[1] == 0
    # the kv length and the positions moved by exactly what was emitted
    assert s.kv_len == kv0 + count and s.tok_pos[0] == pos0 + count


def test_m_zero_leaves_the_draws_alone():
    s = _sample(3, 0, [1, 2, 3, 1, 2])
    s.draft()
    before = list(s.draws)
    n, m = s.step_end([s.ids[1], 7, 7, 7], row_logprob=[-1.0, -2.0, -3.0, -4.0])
    assert m == 0 and s.draws == before == [0, 1, 2, 3] and s.n_out == 0 and s.out_lp == [0.0] * len(s.out_lp)
    # a clipped step: two tokens of room, three accepted - the draws move by the two that were emitted, and so do the log-probabilities
    s = _sample(3, 2, [1, 2, 3, 1, 2], predicted=[4, 4, 4, 4, 4, 4])
    s.draft()
    assert s.n_draft == 3
    n, m = s.step_end([4, 4, 4, 9], row_logprob=[-1.0, -2.0, -3.0, -4.0])
    assert (n, m) == (3, 2) and s.draws == [2, 3, 4, 5] and s.out_lp[:3] == [-1.0, -2.0, 0.0]


def test_the_host_noise_is_the_documented_stream():
    # splitmix64's published test vector (state 0: the first output is splitmix64(0) here, the increment being part of the function)
    assert R.splitmix64(0) == 0xE220A8397B1DCDAF
    key = R.row_key(1234, 7, 3)
    assert key == R.splitmix64(1234 ^ ((7 * 0xD1B54A32D192ED03) & R.MASK) ^ (3 << 32))
    assert R.row_key(1234, 7, 3) != R.row_key(1234, 8, 3) != R.row_key(1234, 8, 4)
    us = [R.uniform(key, n) for n in range(4096)]
    assert all(2.0 ** -24 <= u <= 1.0 - 2.0 ** -24 for u in us)
    assert all((u * 2.0 ** 23 - 0.5).is_integer() for u in us), "u = (r + 0.5) 2^-23 with r an integer below 2^23"
    assert abs(sum(us) / len(us) - 0.5) < 0.02
    g = [R.gumbel(key, n) for n in range(4096)]
    assert abs(sum(g) / len(g) - 0.5772) < 0.06      # the Gumbel mean (Euler's constant), sigma / sqrt(n) = 0.02


def test_the_session_refusals_come_before_any_device_work():
    from unimedvl_amd.sampling import SamplingParams
    from unimedvl_amd.speculative import SpeculativeDecodeSession

    class Cache:
        lens = [3, 4]
    mk = lambda **kw: SpeculativeDecodeSession(None, Cache(), None, None, 4, 2, **kw)      # noqa: E731
    ok = SamplingParams(do_sample=True, temperature=0.8)
    for kw in (dict(sampling=[ok]), dict(sampling=[ok, "x"]), dict(sampling=SamplingParams(repetition_penalty=1.2)),
               dict(sampling=ok, logit_bias={3: 1.0}), dict(sampling=ok, forced_ids=[[0, 0]]), dict(sampling=ok, top_logprobs=2),
               dict(sampling=ok, do_sample=True), dict(sampling=ok, top_k=3), dict(sampling=ok, row_sampling=[ok, ok]),
               dict(sampling_streams=[0, 1])):
        with pytest.raises(ValueError):
            mk(**kw)
    for kw in (dict(row_sampling=[ok, ok]), dict(do_sample=True), dict(logprobs=True)):      # on their own: as before
        with pytest.raises(ValueError, match="greedy only"):
            mk(**kw)
    with pytest.raises(ValueError, match="64"):
        SpeculativeDecodeSession(None, Cache(), None, None, 4, 32, sampling=ok)                # 2 x 33 rows


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_the_rows_step_struct_is_the_c_struct(tmp_path):
    from unimedvl_amd import _lib
    own = ["picks", "rows", "row_logprob", "out_logprobs"]
    step = [n for n, _ in _lib.SpecStepArgs._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(umv_spec_rows_step_args));', '  printf("step_size %zu\\n", sizeof(umv_spec_step_args));']
    lines += [f'  printf("{f} %zu\\n", offsetof(umv_spec_rows_step_args, {f}));' for f in ["step"] + own]
    lines += [f'  printf("step.{f} %zu\\n", offsetof(umv_spec_rows_step_args, step.{f}));' for f in step]
    lines += ["  return 0;", "}"]
    src = tmp_path / "spec_rows_abi.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "spec_rows_abi"
    subprocess.check_call(["gcc", "-std=c11", f"-I{INCLUDE}", "-o", str(exe), str(src)])
    c = {k: int(v) for k, v in (ln.split() for ln in subprocess.check_output([str(exe)], text=True).splitlines())}
    cls = _lib.SpecRowsStepArgs
    assert [n for n, _ in cls._fields_] == ["step"] + own
    assert ctypes.sizeof(cls) == c["size"] and ctypes.sizeof(_lib.SpecStepArgs) == c["step_size"]
    for f in ["step"] + own:
        assert getattr(cls, f).offset == c[f], f
    for f in step:
        assert cls.step.offset + getattr(_lib.SpecStepArgs, f).offset == c["step." + f], f
    assert len(_lib._SIGS["umv_decode_pick_rows"][1]) == 13 and len(_lib._SIGS["umv_decode_step_end_speculative_rows"][1]) == 2
