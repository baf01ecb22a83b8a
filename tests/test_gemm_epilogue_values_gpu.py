"""Every bf16 value through every copy of the GEMM epilogue (csrc/gemm_epilogue.h), against the fp64-per-operation model of
tests/epilogue_ref.py (held to torch on the CPU by tests/test_epilogue_ref_cpu.py).

The other GEMM tests feed Gaussian data and excuse small absolute errors: a wrong rounding point that only shows at a tie, a tail
of an activation, a special value pass them.  Here the fp32 accumulator is made EXACT, so that every output bit is determined:
  * through the weights ("w"): x is one-hot - x[m, 0] = 1, 2 or 0.5 by row, the rest 0 - and W[:, 0] holds the 65 536 bf16 patterns
    in order, so acc[m, n] = x[m, 0] * W[n, 0].  Every such path starts with a baseline case (out_f32, no epilogue) that asserts the
    accumulators themselves, bf16 subnormal weights included (the matrix instruction keeps them: DESIGN.md);
  * through the bias ("b"): zero weights, so acc = +0 exactly, and the bias holds the patterns (0 + b: every pattern arrives, -0 as
    +0).  The route of the entries whose weights cannot carry arbitrary bf16 (e4m3, MXFP4) and of the 13-bit image.
Cases: plain (no flag, bf16(acc): the lean form's KIND 0), bias (the bias a permutation of the patterns by an odd multiplier, so that ties, cancellations and carries occur), residual
with and without bias (a second permutation), GELU-tanh and SiLU on all patterns as pre-activation and on bf16(acc + bias) (epilogue_ref.check_act; the
non-finite inputs must give the class torch gives on the device), OUT_F32, and SwiGLU with gate = all patterns against five up
values - the inner SiLU by check_act, the product bit-exact given the kernel's own inner value.  Everything but the activations is
asserted bit for bit (NaN <-> NaN).

Paths: the weight-streaming kernels of umv_gemm_bf16 at M <= 64 (every launch_skinny instantiation of the default policy, the
for_decode() image, the 33..64-row tile), the tiled kernels at M = 130 under every UMV_GEMM_TILE with the lean and the general
epilogue (one child process per setting, one at a time; TILES says which kernel each setting reaches - the 8-wave tiles need
UMV_GEMM_W4=0, or the 4-wave tiles take their bf16 outputs; umv_gemm_tile_config only echoes a forced setting), umv_gemm_z13w / fp8w / fp8a8w (the sw / sx scale branch) / mxfp4w / mxfp4t,
and the split-K partials.  Each check prints a line "REC {...}" with its counts (profiles/epilogue_values.txt is made of them; with
UMV_EPI_VALUES_LOG=<file> the lines are appended to that file too)."""
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import epilogue_ref as E

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALES = (1.0, 2.0, 0.5)                  # x[m, 0] of row m is SCALES[m % 3]: exact powers of two
UPS = (1.0, -1.0, 1.5703125, 3.3895313892515355e38, 2.0 ** -130)     # SwiGLU up values: +-1, a non-power-of-two, the largest finite, a subnormal
TORCH_ACT = {"silu": F.silu, "gelu_tanh": lambda t: F.gelu(t, approximate="tanh")}
ALL = torch.arange(65536)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    assert not os.environ.get("UMV_GEMM_TILE"), "these tests pin the default policy"
    from unimedvl_amd import ops as o
    return o


def _lib():
    from unimedvl_amd import _lib
    return _lib.load()


def rec(path, case, **kw):
    line = json.dumps(dict(path=path, case=case, **kw))
    print("REC " + line, flush=True)
    log = os.environ.get("UMV_EPI_VALUES_LOG")
    if log:
        with open(log, "a") as f:
            f.write(line + "\n")


def slices_of(n):
    """the 65 536 pattern indices in slices of n columns (the last one wraps round to the first patterns)"""
    return [(torch.arange(n) + s) % 65536 for s in range(0, 65536, n)]


# ---------------------------------------------------------------------------------------------------------- the model, once per process
_cache = {}


def _inputs():
    if "in" not in _cache:
        P, B, R = E.all_bf16(), E.patterns(E.BIAS_MULT, E.BIAS_OFFSET), E.patterns(E.RES_MULT, E.RES_OFFSET)
        _cache["in"] = (P, B, R, P.cuda(), B.cuda(), R.cuda())
    return _cache["in"]


def _acc(inject, s):
    return E.accumulate(s, _inputs()[0]) if inject == "w" else torch.zeros(65536, dtype=torch.float64)


def want_bits(case, inject):
    """[3, 65536] int32 on the device: the expected bits of an exact case for the three row scales"""
    key = (case, inject)
    if key not in _cache:
        P, B, R = _inputs()[:3]
        bias = B if inject == "w" else P
        arg = {"baseline": dict(out_f32=True), "plain": dict(), "bias": dict(bias=bias), "res": dict(residual=R), "bias_res": dict(bias=bias, residual=R),
               "out_f32": dict(bias=bias, out_f32=True)}[case]
        _cache[key] = torch.stack([E.canon_bits(E.epilogue(_acc(inject, s), **arg)[0]) for s in SCALES]).cuda()
    return _cache[key]


def pre_act(inject, permuted_bias=False):
    """[3, 65536] bf16 on the CPU: the pre-activations of the activation cases.  Weights: acc + a zero bias = all patterns, or
    (permuted_bias) bf16(acc + the bias permutation), a sum that has to be rounded BEFORE the activation; bias: 0 + patterns"""
    key = ("pre", inject, permuted_bias)
    if key not in _cache:
        P, B = _inputs()[:2]
        bias = P if inject == "b" else B if permuted_bias else torch.zeros_like(P)
        _cache[key] = torch.stack([E.epilogue(_acc(inject, s), bias)[1] for s in SCALES])
    return _cache[key]


# ---------------------------------------------------------------------------------------------------------- checks
def rows_by_scale(path, case, got, sid):
    """rows with the same x[m, 0] see the same inputs: they must agree bit for bit; returns one row per scale [3, n]"""
    gb = E.canon_bits(got)
    rep = []
    for s in range(3):
        rows = gb[sid == s]
        assert bool((rows == rows[0]).all()), f"{path} {case}: rows with the same inputs differ"
        rep.append(got[int((sid == s).nonzero()[0])])
    return torch.stack(rep)


def check_exact(path, case, got, sid, idx, inject):
    want = want_bits(case, inject)[sid][:, idx.cuda()]
    bad = E.canon_bits(got) != want
    nd = int(bad.sum())
    rec(path, case, checked=got.numel(), differ=nd)
    if nd:
        m, n = [int(v) for v in bad.nonzero()[0]]
        assert False, (f"{path} {case}: {nd} of {got.numel()} values differ from the model, first at row {m} (x = {SCALES[int(sid[m])]}), "
                       f"pattern 0x{int(idx[n]):04x}: got 0x{int(E.canon_bits(got)[m, n]) & 0xFFFFFFFF:x}, want 0x{int(want[m, n]) & 0xFFFFFFFF:x}")


def check_activation(path, case, kind, got_rows, x_rows):
    """got_rows / x_rows [r, n] bf16 (device / CPU): check_act on the finite inputs, torch-on-device's classes on the others"""
    got = got_rows.cpu()
    rep = E.act_report(got, x_rows, kind)
    xd = x_rows.cuda()
    t = TORCH_ACT[kind](xd).cpu()
    nf = ~torch.isfinite(x_rows.float())
    table = sorted(set(zip(E.value_class(x_rows[nf]).tolist(), E.value_class(got[nf]).tolist(), E.value_class(t[nf]).tolist())))
    fin = ~nf
    rec(path, case, checked=got.numel(), finite=rep["finite"], band=rep["band"], differ=rep["differ"], violations=rep["violations"],
        equal_share=round(rep["equal_share"], 6), differ_from_torch_device=int((fin & (E.steps(got, t) != 0)).sum()),
        nonfinite=[f"{E.CLASS_NAMES[a]}->{E.CLASS_NAMES[b]} (torch {E.CLASS_NAMES[c]})" for a, b, c in table])
    assert rep["violations"] == 0, f"{path} {case}: {rep['violations']} inputs break check_act, e.g. x = {rep['worst']}"
    assert rep["equal_share"] >= E.ACT_MIN_EQUAL, f"{path} {case}: only {rep['equal_share']:.5f} bit-equal outside the flush band"
    assert all(b == c for _, b, c in table), f"{path} {case}: classes on non-finite inputs (input, kernel, torch on the device): {table}"


# ---------------------------------------------------------------------------------------------------------- runners
W_CASES = ("baseline", "plain", "bias", "res", "bias_res", "gelu", "silu", "bias_gelu", "bias_silu", "out_f32")
B_CASES = ("bias", "bias_res", "gelu", "silu", "out_f32")


def run_linear(ops, path, M, K, idx_slices, inject, build, cases, **kw):
    """one kernel path through the cases: build(w [n, K], bias [n]) -> PackedLinear; the slices' outputs are joined and checked once"""
    P, B, R, Pd, Bd, Rd = _inputs()
    sid = (torch.arange(M) % 3).cuda()
    x = torch.zeros((M, K), dtype=BF16, device="cuda")
    if inject == "w":
        x[:, 0] = torch.tensor(SCALES, dtype=BF16, device="cuda")[sid]
    else:
        x.fill_(1.0)
    outs = {c: [] for c in cases}
    for idx in idx_slices:
        n, di = len(idx), idx.cuda()
        w = torch.zeros((n, K), dtype=BF16, device="cuda")
        if inject == "w":
            w[:, 0] = Pd[di]
        bias = (Bd if inject == "w" else Pd)[di].contiguous()
        zero_bias = torch.zeros(n, dtype=BF16, device="cuda")
        res = Rd[di].expand(M, n).contiguous()
        lin = build(w, bias)
        for c in cases:
            lin.bias = bias
            if c == "baseline":
                o = ops.gemm(x, lin, out_f32=True, use_bias=False, **kw)
            elif c == "plain":                                  # no flag at all, bf16 out: bf16(acc) (the lean form's KIND 0)
                o = ops.gemm(x, lin, use_bias=False, **kw)
            elif c == "bias":
                o = ops.gemm(x, lin, **kw)
            elif c == "res":
                o = ops.gemm(x, lin, residual=res, use_bias=False, **kw)
            elif c == "bias_res":
                o = ops.gemm(x, lin, residual=res, **kw)
            elif c == "out_f32":
                o = ops.gemm(x, lin, out_f32=True, **kw)
            elif c == "gelu":                                   # (always with a bias: the lean form has GELU only as bias + GELU)
                lin.bias = zero_bias if inject == "w" else bias
                o = ops.gemm(x, lin, act="gelu_tanh", **kw)
            elif c == "silu":
                o = ops.gemm(x, lin, act="silu", use_bias=inject == "b", **kw)
            else:                                               # bias_gelu / bias_silu: acc + bias is not a bf16 value before it is rounded
                o = ops.gemm(x, lin, act="gelu_tanh" if c == "bias_gelu" else "silu", **kw)
            outs[c].append(o)
    idx = torch.cat(idx_slices)
    errors = []
    for c in cases:
        got = torch.cat(outs[c], 1)
        try:
            if c in ("gelu", "silu", "bias_gelu", "bias_silu"):
                kind = "gelu_tanh" if c.endswith("gelu") else "silu"
                check_activation(path, c, kind, rows_by_scale(path, c, got, sid), pre_act(inject, c.startswith("bias_"))[:, idx])
            else:
                check_exact(path, c, got, sid, idx, inject)
        except AssertionError as e:                             # every case of the path is checked and recorded before the test fails
            errors.append(str(e))
    assert not errors, "\n".join(errors)


def run_swiglu(ops, path, M, K, idx_slices, build, **kw):
    """gate = all patterns (x[m, 0] = 1 in every row), up = one value per launch.  up = 1 leaves the kernel's inner bf16(silu(gate)):
    check_act; every other up must give bf16(inner * up) of that very inner value, bit for bit."""
    P, Pd = _inputs()[0], _inputs()[3]
    x = torch.zeros((M, K), dtype=BF16, device="cuda")
    x[:, 0] = 1.0
    sid = torch.zeros(M, dtype=torch.int64, device="cuda")
    outs = {u: [] for u in UPS}
    for idx in idx_slices:
        n = len(idx)
        g = torch.zeros((n, K), dtype=BF16, device="cuda")
        g[:, 0] = Pd[idx.cuda()]
        for u in UPS:
            up = torch.zeros((n, K), dtype=BF16, device="cuda")
            up[:, 0] = u
            outs[u].append(ops.gemm(x, build(g, up), **kw))
    idx = torch.cat(idx_slices)
    gate = E.epilogue(E.accumulate(1.0, P))[1][idx]                 # bf16(acc): the patterns, -0 as +0
    inner, errors = None, []
    for u in UPS:
        got = torch.cat(outs[u], 1)
        gb = E.canon_bits(got)
        assert bool((gb == gb[0]).all()), f"{path} swiglu up={u}: rows with the same inputs differ"
        row = got[0].cpu()
        if inner is None:
            inner = row
            try:
                check_activation(path, "swiglu inner silu (up=1)", "silu", got[:1], gate[None])
            except AssertionError as e:
                errors.append(str(e))
            continue
        want = E.product(inner, torch.full((len(idx),), u, dtype=torch.float64))
        nd = E.count_diff(row, want)
        model = E.swiglu(E.accumulate(1.0, P)[idx], torch.full((len(idx),), u, dtype=torch.float64))[0]
        rec(path, f"swiglu product up={u:g}", checked=row.numel(), differ=nd, differ_from_model=E.count_diff(row, model))
        if nd:
            errors.append(f"{path} swiglu up={u}: {nd} products are not bf16(inner * up) of the kernel's own inner value")
    assert not errors, "\n".join(errors)


def bf16_linear(ops):
    return lambda w, b: ops.PackedLinear.from_weight(w, b)


def bf16_glu(ops):
    return lambda g, u: ops.PackedLinear.from_gate_up(g, u)


# ---------------------------------------------------------------------------------------------------------- umv_gemm_bf16, M <= 64
@pytest.mark.parametrize("M", [3, 16, 20, 32, 40, 64])
def test_skinny_wide_n(ops, M):
    """N = 65 536 (4096 column tiles: the `two` forms of launch_skinny - <1,2,4>, <2,4,2>, <4,4,1> at K < 1024)"""
    assert _lib().umv_gemm_tile_config(M, 65536, 64) == 0
    run_linear(ops, f"bf16 skinny M={M} N=65536 K=64", M, 64, [ALL], "w", bf16_linear(ops), W_CASES)


@pytest.mark.parametrize("M", [3, 16, 20, 32, 40, 64])
def test_skinny_narrow_n(ops, M):
    """N = 4096 slices (256 column tiles: <1,1,8>, <2,1,4,false>, <4,1,4,false>)"""
    run_linear(ops, f"bf16 skinny M={M} N=16x4096 K=64", M, 64, slices_of(4096), "w", bf16_linear(ops), W_CASES)


@pytest.mark.parametrize("M", [3, 16, 20, 32, 40, 64])
def test_skinny_swiglu(ops, M):
    """I = 65 536 (SwiGLU is always a `two` form; 33..64 rows stay on the skinny kernel at K < 1024)"""
    run_swiglu(ops, f"bf16 skinny swiglu M={M} I=65536 K=64", M, 64, [ALL], bf16_glu(ops))


@pytest.mark.parametrize("M", [3, 20, 40])
def test_skinny_decode_image(ops, M):
    """the for_decode() image: N = 3840 = 256 x 15-row tiles, so th = 15 (the `TH != 16` branch, element-wise tile rows)"""
    def build(w, b):
        lin = ops.PackedLinear.from_weight(w, b).for_decode()
        assert lin.th == 15
        return lin
    run_linear(ops, f"bf16 skinny th=15 M={M} N=18x3840 K=64", M, 64, slices_of(3840), "w", build, W_CASES)


@pytest.mark.parametrize("M", [40, 64])
def test_mid_batch_tile(ops, M):
    """33..64 rows on a wide N at K >= 1024: the 128 x 64 LDS-staged tile (launch_tiled<4,1,2,4,1,4,3>), N = 16 384 slices; SwiGLU at
    I = 8192 slices"""
    run_linear(ops, f"bf16 128x64 tile M={M} N=4x16384 K=1024", M, 1024, slices_of(16384), "w", bf16_linear(ops), W_CASES)
    run_swiglu(ops, f"bf16 128x64 tile swiglu M={M} I=8x8192 K=1024", M, 1024, slices_of(8192), bf16_glu(ops))


@pytest.mark.parametrize("M", [3, 20, 40, 100])
def test_splitk_partials_sum_to_the_weights(ops, M):
    """gemm_splitk, S = 2 over K = 64 (launch_skinny<1,4,2>, <2,4,2>, <4,4,1>; 65..128 rows: the 128 x 128 tile): the fp32 partials
    add up to x[m, 0] * W[n, 0] exactly"""
    Pd = _inputs()[3]
    sid = (torch.arange(M) % 3).cuda()
    x = torch.zeros((M, 64), dtype=BF16, device="cuda")
    x[:, 0] = torch.tensor(SCALES, dtype=BF16, device="cuda")[sid]
    w = torch.zeros((65536, 64), dtype=BF16, device="cuda")
    w[:, 0] = Pd
    part = torch.full((2, M, 65536), 7.0, dtype=torch.float32, device="cuda")
    ops.gemm_splitk(x, ops.PackedLinear.from_weight(w), part, 2)
    check_exact(f"bf16 split-K S=2 M={M} N=65536 K=64", "baseline", part[0] + part[1], sid, ALL, "w")


# ---------------------------------------------------------------------------------------------------------- tiled kernels, M = 130
TILED_M, TILED_K = 130, 64
# UMV_GEMM_TILE -> (UMV_GEMM_W4, the kernel the bf16-output cases reach).  With UMV_GEMM_W4 at its default a forced 266 / 268 / 384 is
# handed to the 4-wave tile of the same shape (gemm.hip: 266 -> 366 -> 466, ...) whenever the output is bf16, so the 8-wave tiles are
# walked with UMV_GEMM_W4=0 (as test_gemm_lean_epilogue_bit_identical does) and the 4-wave ones through their own numbers.  Full-line x
# staging (UMV_GEMM_XLINE, default) turns 266 / 268 / 384 / 270 into 366 / 368 / 484 / 370: the same tile shape and epilogue.
TILES = {
    64: ("0", "gemm_tiled_kernel<2,2,4,2,2,3> 128 x 64 x 64, 4 waves"),
    266: ("0", "gemm_tiled_kernel<2,4,8,4,1,4,3> 256 x 256, 8 waves"),
    268: ("0", "gemm_tiled_kernel<4,2,4,4,1,4,3> 256(n) x 128(m), 8 waves"),
    270: ("0", "gemm_tiled_kernel<2,2,4,4,1,4,3> 128 x 128, 4 waves"),
    384: ("0", "gemm_tiled_kernel<4,2,6,4,1,4,3> 384(n) x 128(m), 8 waves: 12 chunks per row, the non-power-of-two LDS addressing"),
    288: ("0", "gemm_tiled_kernel<2,4,9,2,1,4,1> 288(n) x 128(m), 8 waves; SwiGLU: the 8-wave 384 x 128 tile"),
    466: ("1", "gemm_w4 256 x 256, 4 waves, accumulators in AGPRs"),
    468: ("1", "gemm_w4 256(n) x 128(m), 4 waves"),
    4384: ("1", "gemm_w4 384(n) x 128(m), 4 waves"),
}


def tiled_child():
    """all cases under the UMV_GEMM_TILE / UMV_GEMM_LEAN_EPI of this process (both are read once per process)"""
    from unimedvl_amd import ops
    tile, lean = int(os.environ["UMV_GEMM_TILE"]), os.environ["UMV_GEMM_LEAN_EPI"]
    assert _lib().umv_gemm_tile_config(TILED_M, 65536, TILED_K) == tile
    assert os.environ["UMV_GEMM_W4"] == TILES[tile][0]
    path = f"bf16 tiled {tile} [{TILES[tile][1]}] lean={lean} M={TILED_M}"
    # the 4-wave tiles (gemm_w4.hip) refuse fp32 outputs (the policy never sends them one): their accumulators are held by the bf16 cases
    cases = tuple(c for c in W_CASES if c not in ("baseline", "out_f32")) if tile in (466, 468, 4384) else W_CASES
    run_linear(ops, f"{path} N=65536 K=64", TILED_M, TILED_K, [ALL], "w", bf16_linear(ops), cases)
    # a ragged N (the last 16-byte chunk and the last column group are partial): the lean form declines, the general one takes over.
    # The patterns start at 1.0, so that the last columns hold ordinary numbers (0.98..) and not the NaNs the pattern order ends in
    ragged = (torch.arange(65533) + 0x3F80) % 65536
    run_linear(ops, f"{path} N=65533 K=64", TILED_M, TILED_K, [ragged], "w", bf16_linear(ops), ("bias", "bias_res", "bias_gelu"))
    run_swiglu(ops, f"{path} swiglu I=65536 K=64", TILED_M, TILED_K, [ALL], bf16_glu(ops))
    print("OK")


@pytest.mark.parametrize("lean", [1, 0])
@pytest.mark.parametrize("tile", [64, 266, 268, 270, 384, 288, 466, 468, 4384])
def test_tiled(ops, tile, lean):
    code = (f"import sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); "
            "import test_gemm_epilogue_values_gpu as t; t.tiled_child()")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, UMV_GEMM_TILE=str(tile), UMV_GEMM_LEAN_EPI=str(lean), UMV_GEMM_W4=TILES[tile][0]))
    print("\n".join(ln for ln in r.stdout.splitlines() if ln.startswith("REC ")))
    if r.returncode < 0 or r.returncode in (134, 139):      # the child died of a signal: nothing more goes onto this GPU
        pytest.exit(f"tiled child {tile} lean={lean} died with status {r.returncode}: " + r.stderr[-2000:], returncode=3)
    assert r.returncode == 0 and "OK" in r.stdout.splitlines()[-1:], r.stdout[-1500:] + r.stderr[-3000:]


# ---------------------------------------------------------------------------------------------------------- the other entries, by the bias
def test_z13w(ops):
    """umv_gemm_z13w (z13=True): bias, bias + residual, OUT_F32 by the bias; SwiGLU through the weights (the 13-bit image is exact: a
    pattern it cannot hold sends its block to the bf16 image).  A GELU / SiLU call never reaches this entry (ops._route)."""
    run_linear(ops, "z13w M=8 N=65536 K=64", 8, 64, [ALL], "b", lambda w, b: ops.PackedLinear.from_weight(w, b).build_z13(),
               ("bias", "bias_res", "out_f32"), z13=True)
    run_swiglu(ops, "z13w swiglu M=8 I=65536 K=64", 8, 64, [ALL], lambda g, u: ops.PackedLinear.from_gate_up(g, u).build_z13(), z13=True)


def test_fp8w(ops):
    run_linear(ops, "fp8w M=8 N=65536 K=64", 8, 64, [ALL], "b", lambda w, b: ops.PackedLinear.from_weight_fp8(w, b), B_CASES)


def test_fp8a8w(ops):
    """W8A8 on the fp8 matrix instruction: epi_wave_tile_lds with the sw (per column) / sx (per row) scales, 0 * sw * sx + b"""
    run_linear(ops, "fp8a8w (sw / sx) M=130 N=65536 K=64", 130, 64, [ALL], "b",
               lambda w, b: ops.PackedLinear.from_weight_fp8(w, b).enable_fp8_mfma(keep_bf16=True), ("bias", "bias_res", "gelu", "silu"), act8=True)


def test_mxfp4w(ops):
    run_linear(ops, "mxfp4w M=8 N=65536 K=64", 8, 64, [ALL], "b", lambda w, b: ops.PackedLinear.from_weight_mxfp4(w, b), B_CASES)


def test_mxfp4t(ops):
    run_linear(ops, "mxfp4t M=130 N=65536 K=64", 130, 64, [ALL], "b", lambda w, b: ops.PackedLinear.from_weight_mxfp4(w, b, keep_bf16=False), B_CASES)
