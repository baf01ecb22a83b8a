"""The two kernels of the prefill-time scorer on the GPU (include/unimedvl_hip.h, "token log-probabilities of given rows"):
umv_lm_head_stats_bf16 - the lm_head GEMM on an MFMA tile that leaves per-tile softmax statistics and one logit per row instead of
logits - and umv_token_logprob_from_stats, against tests/logprob_ref.py and the plain ops.gemm call on the same x, image and bias.

Bounds, the project's own (tests/test_logprob_gpu.py derives them): the tile maxima equal those of the logits the plain call stored,
exactly; s_t within 1e-5 relative; the finished value within 1e-4 of fp64 for |logprob| <= 200; target_y the plain call's stored logit
at ids[m], bit for bit - whatever tile the plain call took (the shapes at K = 1024 land it on 64, 270, 268 and 384, asserted).
At M = 1 and 64 ops.gemm on M rows takes no tile but the weight-streaming kernel, which sums K in another order and stores about one
logit in 10 000 as the neighbouring bf16 value: there the plain call is made over the same rows repeated past 64 (`_plain`), and a
test of its own compares with the M-row call wherever the two families agree.

Largest errors seen on an MI355X (every test prints its own before it asserts; `pytest -s`): see profiles/score_prefill_tests.txt.
"""
import ctypes as C
import functools
import math

import pytest
import torch

import logprob_ref as R

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
BOUND = 1e-4
GUARD = 3            # guard rows on either side of a workspace
FILL = 7.0
MS = [1, 64, 65, 127, 128, 129, 300]        # one row; both sides of the weight-streaming edge, of one m-block, of two; three m-blocks
# (test_both_sides_of_the_row_count_that_changes_the_tile: 1023, 1024, 1025, 1300)
NS = [330, 1000, 4112]                      # 330: a ragged last tile (10 columns) inside a ragged n-block; 4112: 17 n-blocks, the last of one tile
# (M, N, K, the tile the PLAIN call takes): the statistics kernel has two tiles of its own, the plain call these four - same bits from each
TILE_CASES = [(129, 1000, 1024, 64), (300, 5500, 1024, 270), (512, 12304, 1024, 268), (513, 12304, 1024, 384)]


def _ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from unimedvl_amd import ops
    return ops


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _lin(N, K, special=None):
    """Logits of N(0, ~2.3^2): x ~ N(0, 1), w ~ N(0, (0.1 sqrt(512 / K))^2).  special = "-inf": a bias of -inf on columns 32..47 (a whole
    tile) and 100..103 (part of one); "nan": a NaN bias on column 517"""
    ops = _ops()
    g = torch.Generator().manual_seed(N + K)
    w = (torch.randn(N, K, generator=g) * 0.1 * math.sqrt(512 / K)).to(BF16).cuda()
    b = (torch.randn(N, generator=g) * 0.5).to(BF16)
    if special == "-inf":
        b[32:48] = float("-inf")
        b[100:104] = float("-inf")
    if special == "nan":
        b[517] = float("nan")
    return ops.PackedLinear.from_weight(w, b.cuda())


@functools.lru_cache(maxsize=None)
def _x(K):
    return torch.randn(1300, K, generator=torch.Generator().manual_seed(5)).to(BF16).cuda()


def _ids(M, N):
    return (torch.arange(M, dtype=torch.int64) * 37 % N).cuda()       # every lane group, every tile class, the ragged tile


def _stats(lin, x, ids, M=None):
    """the statistics call on workspaces framed by guard rows -> (lse [M, nt, 2], target_y [M], both with their guards checked)"""
    ops = _ops()
    M = x.shape[0] if M is None else M
    nt = (lin.N + 15) // 16
    rows = x.shape[0]                # the workspaces may hold more rows than the call covers: rows >= M stay as they are
    lse = torch.full((rows + 2 * GUARD, nt, 2), FILL, dtype=torch.float32, device="cuda")
    ty = torch.full((rows + 2 * GUARD,), FILL, dtype=torch.float32, device="cuda")
    ops.lm_head_stats(x, lin, ids, lse[GUARD:], ty[GUARD:], M=M)
    torch.cuda.synchronize()
    for t in (lse, ty):
        assert bool((t[:GUARD] == FILL).all()) and bool((t[GUARD + M:] == FILL).all()), "wrote outside rows [0, M)"
    return lse[GUARD:GUARD + M].clone(), ty[GUARD:GUARD + M].clone()


def _plain(lin, x):
    """The logits the plain ops.gemm call stores for these x rows ON AN MFMA TILE, the family whose bits the statistics kernel has at
    every row count.  Up to 64 rows ops.gemm takes the weight-streaming kernel instead, which cuts K over its 8 waves and adds the
    partial sums in wave order - another order of the same fp32 sum, so about one logit in 10 000 lands on the neighbouring bf16 value
    (measured: 24 of 263 168 at 64 x 4112 x 512, one tile maximum of 16 448 with them).  So the call is made over the same rows
    repeated past 64 - a tile kernel's rows are independent of one another - and the first M rows are taken;
    test_up_to_64_rows_against_the_weight_streaming_call holds the statistics to that other call wherever the two agree."""
    ops = _ops()
    M = x.shape[0]
    if M > 64:
        return ops.gemm(x, lin)
    return ops.gemm(x.repeat((64 + M) // M, 1).contiguous(), lin)[:M].contiguous()


@functools.lru_cache(maxsize=None)
def _case(M, N, K, special=None):
    """one shape, computed once: the plain call's logits, the statistics call's outputs, the finished values"""
    ops = _ops()
    lin, x, ids = _lin(N, K, special), _x(K)[:M], _ids(M, N)
    logits = _plain(lin, x)
    lse, ty = _stats(lin, x, ids)
    out = ops.token_logprob_from_stats(lse, ty, ids, N)
    return logits, lse, ty, out, ids


def _check(M, N, K, special=None):
    """the four bounds of the module docstring for one shape -> (largest relative error of s_t, largest |error| of the finished value)"""
    logits, lse, ty, out, ids = _case(M, N, K, special)
    got = lse.double().cpu()
    assert not bool((lse[..., 1] == FILL).any()), f"M={M} N={N}: a (row, tile) was not written"      # (an s_t is a sum of exponentials: never exactly 7)
    m, s = R.tile_stats(logits)
    assert torch.equal(got[..., 0], m), f"M={M} N={N}: tile maxima differ from the stored logits'"
    rel = ((got[..., 1] - s).abs() / s.clamp_min(1e-300)).max().item()
    assert ((got[..., 1] - s).abs() <= 1e-5 * s).all(), f"M={M} N={N}: s_t off by {rel:.3g} relative"
    assert _same(ty, logits[torch.arange(M, device="cuda"), ids].float()), f"M={M} N={N}: target_y is not the stored logit"
    want = R.logprob(logits, ids)
    fin = torch.isfinite(want)
    err = (out.double().cpu() - want)[fin].abs().max().item()
    assert want[fin].abs().max() <= 200 and err <= BOUND, f"M={M} N={N}: finished value off by {err:.3g}"
    assert torch.equal(out.cpu()[~fin].double(), want[~fin])                                   # a -inf target is -inf, not NaN
    return rel, err


# ----------------------------------------------------------------------------- 1. statistics, target logit and finished value
@pytest.mark.parametrize("N", NS)
def test_stats_and_target_at_every_row_class(N):
    worst = (0.0, 0.0)
    for M in MS:
        worst = tuple(max(a, b) for a, b in zip(worst, _check(M, N, 512)))
    print(f"lm_head stats N={N} K=512: largest relative error of s_t {worst[0]:.3g}, of the finished value {worst[1]:.3g}")


@pytest.mark.parametrize("M,N,K,cfg", TILE_CASES)
def test_same_bits_whatever_tile_the_plain_call_takes(M, N, K, cfg):
    from unimedvl_amd import _lib
    assert _lib.load().umv_gemm_tile_config(M, N, K) == cfg
    rel, err = _check(M, N, K)
    print(f"lm_head stats against tile {cfg} ({M} x {N} x {K}): s_t {rel:.3g} relative, finished value {err:.3g}")


@pytest.mark.parametrize("M", [1, 64])
def test_up_to_64_rows_against_the_weight_streaming_call(M):
    """ops.gemm on M <= 64 rows itself - the weight-streaming kernel, the other summation order (_plain): where it stores a tile's 16
    logits as the tile family does, the statistics kernel's entry for that tile meets the bounds against IT; where it does not, the
    two stored logits are neighbouring bf16 values.  Prints how many differ."""
    ops = _ops()
    differ = 0
    for N in NS:
        lin, x = _lin(N, 512), _x(512)[:M]
        stream, (tiles, lse, ty, out, ids) = ops.gemm(x, lin), _case(M, N, 512)
        a, b = stream.float().cpu(), tiles.float().cpu()
        off = a != b
        differ += int(off.sum())
        # one bf16 ulp at the most - next to 0, where the terms cancel, the error of the fp32 sums themselves (<< 1e-3 at these magnitudes)
        assert ((a - b).abs()[off] <= 2.0 ** -7 * torch.maximum(a.abs(), b.abs())[off] + 1e-3).all()
        nt = (N + 15) // 16
        pad = torch.zeros((M, nt * 16), dtype=torch.bool)
        pad[:, :N] = off
        same_tile = ~pad.reshape(M, nt, 16).any(-1)
        m, s = R.tile_stats(stream)
        got = lse.double().cpu()
        assert torch.equal(got[..., 0][same_tile], m[same_tile]) and ((got[..., 1] - s).abs() <= 1e-5 * s)[same_tile].all()
        same_y = ~off[torch.arange(M), ids.cpu()]
        assert torch.equal(ty.cpu()[same_y], a[torch.arange(M), ids.cpu()][same_y])
        same_row = ~off.any(-1)
        assert ((out.double().cpu() - R.logprob(stream, ids)).abs() <= BOUND)[same_row].all() and bool(same_row.any())
    print(f"M={M}: {differ} stored logits of the weight-streaming call differ from the tile family's (N = {NS}, K = 512)")


@pytest.mark.parametrize("M", [1023, 1024, 1025, 1300])
def test_both_sides_of_the_row_count_that_changes_the_tile(M):
    """from 1024 rows the call takes the 256 x 256 tile (lm_head_stats.hip): the same bounds on either side, a ragged last m-block of 1
    and of 20 rows, and row 3's bits are those of the 65-row call on the other tile"""
    rel, err = _check(M, 330, 512)
    print(f"lm_head stats {M} x 330 x 512: s_t {rel:.3g} relative, finished value {err:.3g}")
    (_, lse, ty, out, _), (_, lse0, ty0, out0, _) = _case(M, 330, 512), _case(65, 330, 512)
    assert _same(lse[3], lse0[3]) and _same(ty[3], ty0[3]) and _same(out[3], out0[3])


# ----------------------------------------------------------------------------- 2. -inf, NaN, ids outside the vocabulary
def test_minus_inf_tiles():
    for M, K in ((65, 512), (129, 1024)):
        _check(M, 1000, K, "-inf")
        logits, lse, ty, out, ids = _case(M, 1000, K, "-inf")
        g = lse.cpu()
        assert not torch.isnan(g).any() and (g[:, 2, 0] == float("-inf")).all() and (g[:, 2, 1] == 0).all()     # the tile of -inf only
        assert (logits[:, 100:104].float() == float("-inf")).all() and torch.isfinite(g[:, 6]).all()              # the partial one
        assert not torch.isnan(out).any() and out[1] == float("-inf") and torch.isfinite(out[0])                # row 1's target, column 37, is -inf
        # every target inside the -inf tile: -inf, not NaN
        ops, forced = _ops(), torch.full((M,), 40, dtype=torch.int64, device="cuda")
        lse2, ty2 = _stats(_lin(1000, K, "-inf"), _x(K)[:M], forced)
        assert _same(lse2, lse) and (ops.token_logprob_from_stats(lse2, ty2, forced, 1000) == float("-inf")).all()


def test_nan_logits():
    ops = _ops()
    M, N, K = 70, 1000, 512
    ids = _ids(M, N)
    # a NaN column (through the bias): every row is NaN
    lse, ty = _stats(_lin(N, K, "nan"), _x(K)[:M], ids)
    assert torch.isnan(lse[:, 517 // 16, 1]).all() and int(torch.isnan(lse[..., 1]).sum()) == M
    assert torch.isnan(ops.token_logprob_from_stats(lse, ty, ids, N)).all()
    # a NaN in one x row: that row is NaN, the others keep their bits
    x = _x(K)[:M].clone()
    x[4, 9] = float("nan")
    lse, ty = _stats(_lin(N, K), x, ids)
    out = ops.token_logprob_from_stats(lse, ty, ids, N)
    _, lse0, ty0, out0, _ = _case(M, N, K)
    others = [r for r in range(M) if r != 4]
    assert math.isnan(out[4]) and _same(out[others], out0[others]) and _same(lse[others], lse0[others]) and _same(ty[others], ty0[others])


def test_ids_outside_the_vocabulary():
    ops = _ops()
    M, N, K = 66, 330, 512
    ids = _ids(M, N)
    ids[3], ids[65], ids[20] = -1, N, N - 1           # below, above (the padding of the ragged tile holds a column N), the last column
    lse, ty = _stats(_lin(N, K), _x(K)[:M], ids)
    out = ops.token_logprob_from_stats(lse, ty, ids, N).cpu()
    assert math.isnan(out[3]) and math.isnan(out[65]) and ty[3] == FILL and ty[65] == FILL       # no logit is written for them
    logits = ops.gemm(_x(K)[:M], _lin(N, K))
    keep = [r for r in range(M) if r not in (3, 65)]
    want = R.logprob(logits[keep], ids[keep])
    assert (out[keep].double() - want).abs().max() <= BOUND and ty[20] == logits[20, N - 1].float()


# ----------------------------------------------------------------------------- 3. what is written
def test_rows_beyond_m_are_not_written():
    """workspaces of 300 rows, a call over the first 129: rows 129.. keep the prefill (the guards are checked by _stats)"""
    N, K = 1000, 512
    lse, ty = _stats(_lin(N, K), _x(K)[:300], _ids(300, N), M=129)
    _, lse0, ty0, _, _ = _case(129, N, K)
    assert _same(lse, lse0) and _same(ty, ty0)


# ----------------------------------------------------------------------------- 4. row independence
def test_a_rows_bits_do_not_depend_on_the_call():
    """row 3 of a 65-row call, row 3 of a 300-row call and row 200 of that call (another m-block, another wave row) fed the same x row and
    the same target: the same statistics, target logit and result, bit for bit; the same call twice: the same bits"""
    ops = _ops()
    N, K = 4112, 512
    lin = _lin(N, K)
    x = _x(K)[:300].clone()
    x[200] = x[3]
    ids = _ids(300, N)
    ids[200] = ids[3]

    def run(M):
        lse, ty = _stats(lin, x[:M], ids[:M].contiguous())
        return lse, ty, ops.token_logprob_from_stats(lse, ty, ids[:M].contiguous(), N)
    a, b, again = run(65), run(300), run(300)
    for what, ta, tb in zip(("statistics", "target_y", "result"), a, b):
        assert _same(ta[3], tb[3]), f"row 3 of 65 vs of 300: {what}"
        assert _same(tb[3], tb[200]), f"row 3 vs row 200 of 300: {what}"
    assert all(_same(p, q) for p, q in zip(b, again))


# ----------------------------------------------------------------------------- 5. the finish kernel against the decode step end
@pytest.mark.parametrize("M", [8, 64])
def test_finish_equals_the_decode_step_end(M):
    """the weight-streaming lm_head call with lse_partial, then decode_step_end_logprob with forced ids; the new finish on the same
    statistics, with y gathered from the stored logits: that kernel's bits"""
    ops = _ops()
    N, K = 4112, 512
    nt = (N + 15) // 16
    keys = torch.zeros((M, nt), dtype=torch.int64, device="cuda")
    st = torch.full((M, nt, 2), FILL, dtype=torch.float32, device="cuda")
    logits = torch.empty((M, N), dtype=BF16, device="cuda")
    ops.gemm(_x(K)[:M], _lin(N, K), out=logits, argmax_partial=keys, lse_partial=st)
    ids = _ids(M, N)
    dev = "cuda"
    lp = torch.full((2, M), 99.0, dtype=torch.float32, device=dev)
    i32 = lambda: torch.zeros(M, dtype=torch.int32, device=dev)           # noqa: E731
    ops.decode_step_end_logprob(i32(), i32(), i32(), keys, st, torch.zeros(M, dtype=torch.int64, device=dev),
                                torch.zeros((2, M), dtype=torch.int64, device=dev), torch.zeros((2, M), dtype=torch.int64, device=dev),
                                torch.zeros(M, dtype=torch.int64, device=dev), logits, lp, temperature=0.0,
                                forced_ids=torch.stack([ids, ids]).contiguous())
    ty = logits[torch.arange(M, device=dev), ids].float()
    assert not bool((st[..., 1] == FILL).any()) and not bool((lp[0] == 99.0).any())
    assert _same(ops.token_logprob_from_stats(st, ty, ids, N), lp[0])


# ----------------------------------------------------------------------------- 6. refused arguments launch nothing
def test_refused_arguments():
    ops = _ops()
    from unimedvl_amd import _lib
    lib = _lib.load()
    M, N, K = 70, 1000, 512
    lin, x, ids = _lin(N, K), _x(K)[:M], _ids(M, N)
    nt = (N + 15) // 16
    lse = torch.full((M, nt, 2), FILL, dtype=torch.float32, device="cuda")
    ty = torch.full((M,), FILL, dtype=torch.float32, device="cuda")
    other = torch.zeros((M, N), dtype=BF16, device="cuda")
    words = torch.zeros((M, nt), dtype=torch.int64, device="cuda")

    def call(ids_p=ids, lse_p=lse, ty_p=ty, **fields):
        a = _lib.GemmArgs(x=x.data_ptr(), ldx=x.stride(0), wp=lin.wp.data_ptr(), bias=lin.bias.data_ptr(), M=M, N=N, K=K, epilogue=_lib.EPI_BIAS)
        for k, v in fields.items():
            setattr(a, k, v)
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())       # noqa: E731
        return lib.umv_lm_head_stats_bf16(C.byref(a), p(ids_p), p(lse_p), p(ty_p), None)
    ARG, UNSUPPORTED = -1, -3
    cases = [("row_idx", dict(row_idx=words.data_ptr()), UNSUPPORTED), ("residual", dict(residual=other.data_ptr(), ldr=N), UNSUPPORTED),
             ("k_splits", dict(k_splits=2, split_stride=M * N), UNSUPPORTED), ("norm_w", dict(norm_w=other.data_ptr()), UNSUPPORTED),
             ("tile_rows", dict(tile_rows=8), UNSUPPORTED), ("gelu", dict(epilogue=_lib.EPI_BIAS | _lib.EPI_GELU_TANH), UNSUPPORTED),
             ("silu", dict(epilogue=_lib.EPI_SILU), UNSUPPORTED), ("out_f32", dict(epilogue=_lib.EPI_OUT_F32), UNSUPPORTED),
             ("residual flag", dict(epilogue=_lib.EPI_RESIDUAL, residual=other.data_ptr(), ldr=N), UNSUPPORTED),
             ("swiglu", dict(epilogue=_lib.EPI_SWIGLU), None), ("argmax_partial", dict(argmax_partial=words.data_ptr()), UNSUPPORTED),
             ("sample_temperature", dict(sample_temperature=0.7), UNSUPPORTED), ("lse_partial in the struct", dict(lse_partial=lse.data_ptr()), ARG),
             ("no ids", dict(ids_p=None), ARG), ("no lse_partial", dict(lse_p=None), ARG), ("no target_y", dict(ty_p=None), ARG),
             ("no x", dict(x=None), ARG), ("K % 8", dict(K=508), ARG)]
    for name, kw, want in cases:
        rc = call(**kw)
        assert rc in (ARG, UNSUPPORTED) and (want is None or rc == want), f"{name}: rc={rc}"
        assert lib.umv_last_error()
    torch.cuda.synchronize()
    assert bool((lse == FILL).all()) and bool((ty == FILL).all()), "a refused call launched"
    assert call() == 0 and call(out=other.data_ptr(), ldo=N) == 0        # the same struct is accepted, without `out` and with one (ignored)
    torch.cuda.synchronize()
    assert not bool(other.any())
    torch.cuda.synchronize()
    assert not bool((lse[..., 1] == FILL).any())
    # the finish
    out = torch.full((M,), FILL, dtype=torch.float32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())                               # noqa: E731
    assert lib.umv_token_logprob_from_stats(None, nt, p(ty), p(ids), N, p(out), M, None) == ARG
    assert lib.umv_token_logprob_from_stats(p(lse), nt, p(ty), p(ids), N + 16, p(out), M, None) == ARG     # V is not behind these tiles
    assert lib.umv_token_logprob_from_stats(p(lse), nt, p(ty), p(ids), N - 16, p(out), M, None) == ARG
    torch.cuda.synchronize()
    assert bool((out == FILL).all())
    # the wrappers refuse what the kernels cannot take
    with pytest.raises(_lib.UmvError, match="plain bf16"):
        ops.lm_head_stats(x, ops.PackedLinear.from_weight_fp8(torch.zeros((64, K), dtype=BF16, device="cuda")), ids, lse, ty)
    with pytest.raises(_lib.UmvError, match="lse_partial"):
        ops.lm_head_stats(x, lin, ids, lse[:, :10].contiguous(), ty)
