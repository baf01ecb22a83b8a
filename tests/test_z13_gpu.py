"""The exact 13-bit weight image "z13" on the GPU:
  * umv_pack_weight_z13 == tests/z13_ref.py byte for byte (flags, bases, the records of every block that is not flagged);
  * umv_gemm_z13w == umv_gemm_bf16 bit for bit - every row-count class, K splits whose wave slices start on odd 32-k tiles, every
    epilogue - on clean images, on images with flagged blocks (the workgroups that meet one run the bf16 body) and on images where
    every block is flagged;
  * the engine with the images on against off: the same logits and ids, bit for bit, over 16 greedy steps under the graph."""
import copy
import functools

import numpy as np
import pytest
import torch

import z13_ref as z
from conftest import NEW_TOKEN_IDS

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
MS = [1, 7, 8, 9, 16, 17, 32, 64]


def _ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from unimedvl_amd import ops
    return ops


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _w(N, K, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(N, K, generator=g) * 0.02).to(BF16)


def _np16(t):
    return t.cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def _flags(lin):
    ntt = (lin.N + 15) // 16
    return z.split_bytes(lin.wz.cpu().numpy(), lin.N, lin.K)[0], (ntt + 1) // 2, (lin.K + 511) // 512


def _twin(lin):
    ops = _ops()
    return ops.PackedLinear(lin.wp, lin.bias, lin.N, lin.K, swiglu=lin.swiglu)


PLANTS = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf"), "2^-40": 2.0 ** -44, "subnormal": 2.0 ** -130,
          "+0": 0.0, "-0": -0.0}        # 2^-44: the largest of ~1e5 N(0, 0.02^2) draws is in [2^-4, 2^-3): 40 binades below it


@functools.lru_cache(maxsize=None)
def _lin(N, K, kind="clean"):
    """kind: clean | swiglu | planted (one weight of each PLANTS kind in pair 1, all inside k = [1792, 2304) - with K = 3584 and 4
    splits of 896 that is split 2 alone, 512-k blocks 3 and 4) | allflag (a zero in every (pair, 512-k block))"""
    ops = _ops()
    if kind == "swiglu":
        lin = ops.PackedLinear.from_gate_up(_w(N // 2, K, N + K).cuda(), _w(N // 2, K, N + K + 1).cuda())
        return lin.build_z13()
    w = _w(N, K, N + K)
    if kind == "planted":
        for i, v in enumerate(PLANTS.values()):
            w[32 + 3 * i, 1800 + 61 * i] = v
    if kind == "allflag":
        w[3::32, 7::512] = 0.0
    b = (torch.randn(N, generator=torch.Generator().manual_seed(N)) * 0.1).to(BF16)
    return ops.PackedLinear.from_weight(w.cuda(), b.cuda()).build_z13()


# ----------------------------------------------------------------------------- the packer
@pytest.mark.parametrize("N,K,kind", [(80, 576, "clean"), (128, 3584, "planted"), (128, 3584, "allflag"), (64, 512, "swiglu"),
                                      (40, 128, "clean")])
def test_device_pack_matches_restatement(N, K, kind):
    lin = _lin(N, K, kind)
    ntt = (N + 15) // 16
    img16 = _np16(lin.wp).reshape(ntt, K // 32, 64, 8)
    if kind == "swiglu":
        want = z.bf16_image_swiglu(_np16(_w(N // 2, K, N + K)), _np16(_w(N // 2, K, N + K + 1)))
    else:
        w = _w(N, K, N + K)
        if kind == "planted":
            for i, v in enumerate(PLANTS.values()):
                w[32 + 3 * i, 1800 + 61 * i] = v
        if kind == "allflag":
            w[3::32, 7::512] = 0.0
        want = z.bf16_image(_np16(w))
    assert np.array_equal(img16, want)                      # the restatement's bf16 image is the device's
    flags, bases, rec, flagged = z.pack(img16, N)
    assert lin.wz.numel() == z.image_bytes(N, K)
    dflags, dbases, drec = z.split_bytes(lin.wz.cpu().numpy(), N, K)
    assert np.array_equal(dflags, flags) and np.array_equal(dbases, bases)
    keep = ~np.repeat(flagged, 8, axis=1)[:, :rec.shape[1]]              # [pair, unit]: contents of flagged blocks are unspecified
    assert np.array_equal(drec[keep], rec[keep])
    if kind == "clean" or kind == "swiglu":
        assert not flagged.any()
        assert np.array_equal(z.unpack(dbases, drec, ntt)[:N // 16], img16[:N // 16])
    if kind == "planted":
        assert flagged.tolist() == [[False] * 7, [False, False, False, True, True, False, False], [False] * 7, [False] * 7]
    if kind == "allflag":
        assert flagged.all()


# ----------------------------------------------------------------------------- bit identity
def _epilogues(ops, lin, x, M):
    """every epilogue of one linear on x's first M rows -> list of (name, tensors).  z13=True: every call on a linear with the image goes
    to umv_gemm_z13w, not only the forms the engine routes there"""
    N = lin.N
    real = ops.gemm

    class Forced:
        @staticmethod
        def gemm(*a, **kw):
            return real(*a, z13=True, **kw)
    ops = Forced
    g = torch.Generator().manual_seed(M)
    res = torch.randn(x.shape[0], N, generator=g).to(BF16).cuda()
    idx = torch.randperm(x.shape[0], generator=g)[:M].to(torch.int32).cuda()
    out = []
    o = torch.full((M, N), 7.0, dtype=BF16, device="cuda")
    ops.gemm(x[:M], lin, out=o, use_bias=False)
    out.append(("plain", [o]))
    out.append(("bias", [ops.gemm(x[:M], lin)]))
    o = res[:M].clone()
    ops.gemm(x[:M], lin, out=o, residual=o)
    out.append(("residual", [o]))
    out.append(("f32", [ops.gemm(x[:M], lin, out_f32=True)]))
    o = res.clone()
    ops.gemm(x, lin, out=o, M=M, residual=o, row_idx=idx)
    out.append(("row_idx", [o]))
    for name, sample in (("argmax", None), ("sampling keys", (0.7, 1234, None))):
        keys = torch.zeros((M, (N + 15) // 16), dtype=torch.int64, device="cuda")
        o = ops.gemm(x[:M], lin, argmax_partial=keys, sample=sample)
        out.append((name, [o, keys]))
    return out


def _x(M, K, seed=0):
    rows = max(M, 8) + 3
    return torch.randn(rows, K, generator=torch.Generator().manual_seed(1000 * M + seed)).to(BF16).cuda()


def _check_all_epilogues(lin, M):
    ops = _ops()
    x = _x(M, lin.K)
    got, ref = _epilogues(ops, lin, x, M), _epilogues(ops, _twin(lin), x, M)
    for (name, a), (_, b) in zip(got, ref):
        for ta, tb in zip(a, b):
            if ta.dtype == torch.int64:
                assert torch.equal(ta, tb), f"{name} M={M}"
            else:
                assert _same(ta, tb), f"{name} M={M}"


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N,K", [(64, 512), (80, 576), (128, 3584)])
def test_gemm_bit_identical_every_epilogue(M, N, K):
    """(80, 576): a ragged last pair (5 tiles) and 18 k-tiles over 8 waves = slices of 3 - odd starts, two empty waves"""
    lin = _lin(N, K)
    assert not _flags(lin)[0].any()
    _check_all_epilogues(lin, M)


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N,K", [(64, 512), (128, 3584)])
def test_gemm_swiglu_bit_identical(M, N, K):
    """(SwiGLU needs N % 32 == 0: not the 80-column shape.)  At 33..64 rows and K >= 1024 umv_gemm_bf16 runs an MFMA tile with one
    accumulator chain; umv_gemm_z13w hands those calls to it, so they are equal as well."""
    ops = _ops()
    lin = _lin(N, K, "swiglu")
    x = _x(M, K, 1)
    assert _same(ops.gemm(x[:M], lin, z13=True), ops.gemm(x[:M], _twin(lin)))


def _splitk(ops, lin, x, M, S):
    p = torch.full((S, M, lin.N), float("nan"), dtype=torch.float32, device="cuda")
    ops.gemm_splitk(x[:M], lin, p, S, z13=True)
    return p


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N,K,S,kind", [(128, 3584, 3, "clean"), (128, 3584, 4, "clean"), (64, 18944, 4, "clean"),
                                        (128, 3584, 4, "planted"), (128, 3584, 3, "allflag")])
def test_splitk_partials_bit_identical(M, N, K, S, kind):
    """(64, 18944) / 4: 148 k-tiles per split, wave slices of 19 - every other one starts in the middle of a 64-k unit; (128, 3584) / 3:
    38 tiles per split (the third has 36), slices of 5.  planted: only split 2 of pair 1 meets a flag."""
    ops = _ops()
    lin = _lin(N, K, kind)
    x = _x(M, K, S)
    got, ref = _splitk(ops, lin, x, M, S), _splitk(ops, _twin(lin), x, M, S)
    assert _same(got, ref)
    if kind == "clean":
        assert torch.isfinite(got).all()


@pytest.mark.parametrize("M", [8, 17, 64])
@pytest.mark.parametrize("kind", ["planted", "allflag"])
def test_flagged_images_bit_identical_every_epilogue(M, kind):
    lin = _lin(128, 3584, kind)
    flags, NP, nblk = _flags(lin)
    if kind == "allflag":
        assert all(int(f) == (1 << nblk) - 1 for f in flags)
    else:
        assert [int(f) for f in flags] == [0, 0b0011000, 0, 0]
    _check_all_epilogues(lin, M)


def test_argument_rejection():
    import ctypes as C
    from unimedvl_amd import _lib
    ops = _ops()
    lib = _lib.load()
    lin = _lin(64, 512)
    x = torch.randn(80, 512, device="cuda").to(BF16)
    out = torch.empty(80, 64, dtype=BF16, device="cuda")

    def call(z13=lin.wz.data_ptr(), **kw):
        a = dict(x=x.data_ptr(), ldx=512, wp=lin.wp.data_ptr(), out=out.data_ptr(), ldo=64, M=8, N=64, K=512, epilogue=0)
        a.update(kw)
        return _lib.check(lib.umv_gemm_z13w(C.byref(_lib.GemmArgs(**a)), z13, ops._stream()), "umv_gemm_z13w")

    call()
    with pytest.raises(_lib.UmvError, match="M <= 64"):
        call(M=65)
    with pytest.raises(_lib.UmvError, match="multiple of 64"):
        call(K=480)
    with pytest.raises(_lib.UmvError, match="fused norm"):
        call(norm_w=x.data_ptr())
    with pytest.raises(_lib.UmvError, match="fused norm / th-row"):
        call(tile_rows=14)
    with pytest.raises(_lib.UmvError, match="null pointer"):
        call(z13=None)
    with pytest.raises(_lib.UmvError, match="multiple of 64"):
        ops.PackedLinear.from_weight(torch.zeros(16, 96, dtype=BF16, device="cuda")).build_z13()
    # above 64 rows ops.gemm takes the bf16 image, forced or not
    assert _same(ops.gemm(x, lin, z13=True), ops.gemm(x, _twin(lin)))


def test_routing_policy(monkeypatch):
    """without z13=True only the decode forms and row counts that were measured and won reach umv_gemm_z13w"""
    ops = _ops()
    taken = []
    real = ops._z13_takes
    monkeypatch.setattr(ops, "_z13_takes", lambda *a, **kw: taken.append(real(*a, **kw)) or taken[-1])
    lin, sw = _lin(64, 512), _lin(64, 512, "swiglu")
    x = _x(64, 512)
    # (rows, SwiGLU / keys, split-K): 9..16 rows of gate/up and lm_head only tie with the bf16 kernel and stay on it
    for M, want, want_split in ((8, True, True), (9, False, True), (16, False, True), (17, True, True), (32, True, True),
                                (33, False, False), (64, False, False)):
        keys = torch.zeros((M, 4), dtype=torch.int64, device="cuda")
        p = torch.empty((2, M, 64), dtype=torch.float32, device="cuda")
        taken.clear()
        ops.gemm(x[:M], sw)
        ops.gemm(x[:M], lin, argmax_partial=keys)
        ops.gemm_splitk(x[:M], lin, p, 2)
        assert taken == [want, want, want_split], (M, taken)
        taken.clear()
        ops.gemm(x[:M], lin)                                # plain / bias: not a decode form
        ops.gemm(x[:M], lin, out_f32=True)
        ops.gemm(x[:M], sw, z13=False)
        assert taken == [False] * 3, (M, taken)
        taken.clear()
        ops.gemm(x[:M], lin, z13=True)
        assert taken == [True]


# ----------------------------------------------------------------------------- the engine
def test_engine_on_equals_off_under_the_graph(tiny_weights, monkeypatch):
    ops = _ops()
    taken = []
    real = ops._z13_takes
    monkeypatch.setattr(ops, "_z13_takes", lambda *a, **kw: taken.append(real(*a, **kw)) or taken[-1])
    from unimedvl_amd.bagel import Bagel
    from unimedvl_amd.config import UniMedVLConfig
    from unimedvl_amd.decode import DecodeSession
    from unimedvl_amd.kvcache import NaiveCache
    cfg, sd, _, _ = tiny_weights
    prompts = [[11, 22, 33, 44, 55], [66, 77, 88]]

    class Tok:
        def encode(self, s):
            return prompts[int(s)]

    runs = []
    for on in (True, False):
        c = copy.deepcopy(UniMedVLConfig.from_dict(cfg))
        c.llm_decode_z13 = on
        model = Bagel(c, lambda n: sd[n], device="cuda")
        w = model.language_model.w
        has = [lin.wz is not None for lin in [w.lm_head] + [l for lw in w.und for l in (lw.gate_up, lw.down)]]
        assert all(has) if on else not any(has)
        assert all(lw.qkv.wz is None and lw.o.wz is None for lw in w.und)
        if on:
            bf16_bytes = sum(l.nbytes() for lw in w.und for l in (lw.qkv, lw.o, lw.gate_up, lw.down)) + w.lm_head.nbytes()
            assert w.decode_weight_bytes() < bf16_bytes
        cache = NaiveCache(cfg["layers"])
        gi, kvl, rope = model.prepare_prompts([0, 0], [0, 0], ["0", "1"], Tok(), NEW_TOKEN_IDS)
        cache = model.forward_cache_update_text(cache, **gi)
        gi = model.prepare_start_tokens(kvl, rope, NEW_TOKEN_IDS)
        with torch.no_grad():
            sess = DecodeSession(model.language_model, cache, gi["packed_start_tokens"], gi["packed_query_position_ids"], 16,
                                 use_graph=True)
            assert sess.graph is not None
            # the step's gate/up, down (split-K) and lm_head (argmax keys) GEMMs stream the image when it is there
            assert sum(taken) >= (2 * cfg["layers"] + 1 if on else 0) and (on or not any(taken))
            taken.clear()
            logits = []
            for _ in range(16):
                sess.step(1)
                logits.append(sess.logits.clone())
            runs.append((torch.stack(logits), sess.pred_ids[:16].clone()))
    assert _same(runs[0][0], runs[1][0])
    assert torch.equal(runs[0][1], runs[1][1])
