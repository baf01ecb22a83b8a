"""The MFMA-tiled GEMM on the MXFP4 image (umv_gemm_mxfp4t, M > 64) and the fp4 mode that stands on it (llm_fp4_keep_bf16=False):
  * the kernel == umv_gemm_bf16 on the bf16 image of W', torch.equal, every shape / epilogue / row_idx, split-K partials included - W' is
    exact in bf16 and both kernels run one v_mfma_f32_16x16x32_bf16 chain per output over k in ascending 32-wide steps, so there is no
    tolerance anywhere in this file;
  * argument rejection;
  * the engine without the bf16 images == the engine that carries them, bit for bit (prefill, decode, flow passes, 96-sample decode);
  * the memory the dropped images give back, and the packed file of the standalone mode."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import NEW_TOKEN_IDS
from test_mxfp4_gpu import _bf16_twin, _lin, _ops, _weights

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16

MODEL_SHAPES = [(4608, 3584, False), (3584, 3584, False), (2 * 18944, 3584, True), (3584, 18944, False)]


def _alone(lin):
    """the same linear without its bf16 image: above 64 rows ops.gemm / ops.gemm_splitk can only take umv_gemm_mxfp4t"""
    ops = _ops()
    return ops.PackedLinear(None, lin.bias, lin.N, lin.K, swiglu=lin.swiglu, w4=lin.w4)


def _x(M, K, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(M, K, device="cuda", generator=g).to(BF16)


@pytest.mark.parametrize("M", [65, 100, 128, 129, 272, 1060, 2048, 8480])
@pytest.mark.parametrize("N,K,swiglu", MODEL_SHAPES)
def test_tiled_gemm_bit_identical_to_bf16_on_dequantised_weights(M, N, K, swiglu):
    ops = _ops()
    lin = _lin(N, K, swiglu)
    x = _x(M, K, M)
    out = ops.gemm(x, _alone(lin))
    ref = ops.gemm(x, _bf16_twin(lin))
    assert torch.isfinite(out.float()).all() and out.abs().max() > 0
    assert torch.equal(out, ref)


@pytest.mark.parametrize("M", [65, 128, 129, 272])
@pytest.mark.parametrize("N,K", [(200, 1056), (48, 96), (3584, 3584)])
def test_tiled_gemm_ragged_shapes_and_special_blocks(M, N, K):
    """K not a multiple of 64, N not a multiple of 32; weights with all-zero blocks, -0 codes and the clamped exponents"""
    ops = _ops()
    lin = ops.PackedLinear.from_weight_mxfp4(_weights(N, K, N * 7 + K).cuda())
    x = _x(M, K, M + N)
    out = ops.gemm(x, _alone(lin), out_f32=True)
    ref = ops.gemm(x, _bf16_twin(lin), out_f32=True)
    assert torch.isfinite(out).all()
    assert torch.equal(out, ref)
    assert torch.equal(ops.gemm(x, _alone(lin)), ops.gemm(x, _bf16_twin(lin)))


@pytest.mark.parametrize("M", [100, 300])
def test_tiled_gemm_epilogues_and_row_idx(M):
    ops = _ops()
    lin = _lin(4608, 3584, False)
    g = torch.Generator(device="cuda").manual_seed(9)
    rows = 2 * M + 7
    x = torch.randn(rows, 3584, device="cuda", generator=g).to(BF16)
    res = torch.randn(rows, 4608, device="cuda", generator=g).to(BF16)
    idx = (torch.randperm(rows, generator=torch.Generator().manual_seed(M))[:M]).to(torch.int32).cuda()      # a permutation with gaps
    outs = []
    for l in (_alone(lin), _bf16_twin(lin)):
        o = res.clone()
        ops.gemm(x, l, out=o, M=M, residual=o, row_idx=idx)                  # BIAS + RESIDUAL + row_idx
        f = ops.gemm(x[:M], l, out_f32=True, use_bias=False)                 # OUT_F32, no bias
        fb = ops.gemm(x[:M], l, out_f32=True)                                # OUT_F32 + BIAS
        b = ops.gemm(x[:M], l)                                               # BIAS
        r = ops.gemm(x[:M], l, residual=res[:M], use_bias=False)             # RESIDUAL
        s = ops.gemm(x[:M], l, act="silu")                                   # BIAS + SILU
        outs.append((o, f, fb, b, r, s))
    for got, ref in zip(*outs):
        assert torch.equal(got, ref)
    untouched = torch.ones(rows, dtype=torch.bool)
    untouched[idx.cpu().long()] = False
    assert torch.equal(outs[0][0][untouched.cuda()], res[untouched.cuda()])
    # SwiGLU with row_idx (the MoT routing of the flow passes)
    lg = _lin(2 * 18944, 3584, True)
    oo = []
    for l in (_alone(lg), _bf16_twin(lg)):
        o = torch.zeros(rows, 18944, dtype=BF16, device="cuda")
        ops.gemm(x, l, out=o, M=M, row_idx=idx)
        oo.append(o)
    assert torch.equal(oo[0], oo[1]) and oo[0].abs().max() > 0


@pytest.mark.parametrize("M", [65, 96, 128])
@pytest.mark.parametrize("N,K,S", [(4608, 3584, 6), (3584, 3584, 8), (3584, 18944, 8), (256, 384, 8)])
def test_tiled_splitk_partials(M, N, K, S):
    """every split's raw fp32 partial, also the empty ones: (256, 384, 8) is 12 k-tiles in ranges of 2 - splits 6 and 7 hold zeros"""
    ops = _ops()
    lin = _lin(N, K, False)
    x = _x(M, K, M + S)
    p = torch.full((S, M, N), float("nan"), dtype=torch.float32, device="cuda")
    ops.gemm_splitk(x, _alone(lin), p, S)
    p16 = torch.full((S, M, N), float("nan"), dtype=torch.float32, device="cuda")
    ops.gemm_splitk(x, ops.PackedLinear(lin.wp, None, lin.N, lin.K), p16, S)
    assert torch.isfinite(p).all()
    for s in range(S):
        assert torch.equal(p[s], p16[s]), f"split {s}"
    if (N, K, S) == (256, 384, 8):
        assert p[6:].abs().max() == 0 and p[5].abs().max() > 0


def test_tiled_gemm_argument_rejection():
    from unimedvl_amd import _lib
    ops = _ops()
    lib = _lib.load()
    lin = _lin(200, 1024, False)
    x = torch.randn(80, 1024, device="cuda").to(BF16)
    out = torch.full((80, 200), 7.0, dtype=BF16, device="cuda")

    def call(**kw):
        a = dict(x=x.data_ptr(), ldx=1024, wp=lin.w4.data_ptr(), out=out.data_ptr(), ldo=200, M=80, N=200, K=1024, epilogue=0)
        a.update(kw)
        return _lib.check(lib.umv_gemm_mxfp4t(C.byref(_lib.GemmArgs(**a)), ops._stream()), "umv_gemm_mxfp4t")

    with pytest.raises(_lib.UmvError, match="umv_gemm_mxfp4w"):
        call(M=64)
    with pytest.raises(_lib.UmvError, match="w_scale must be NULL"):
        call(w_scale=out.data_ptr())
    with pytest.raises(_lib.UmvError, match="fused norm.*umv_gemm_bf16"):
        call(norm_w=x.data_ptr())
    amax = torch.zeros(80, 13, dtype=torch.int64, device="cuda")
    with pytest.raises(_lib.UmvError, match="argmax_partial.*umv_gemm_fp8w"):
        call(argmax_partial=amax.data_ptr())
    with pytest.raises(_lib.UmvError, match="multiple of 32"):
        call(K=1000)
    with pytest.raises(_lib.UmvError, match="th-row tiles"):
        call(tile_rows=8)
    torch.cuda.synchronize()
    assert (out == 7.0).all(), "a rejected call must not launch"
    call()
    assert torch.equal(out, ops.gemm(x, _bf16_twin(lin), use_bias=False))
    # the Python layer names fp4 when a standalone linear is asked for what only the bf16 image can do
    with pytest.raises(_lib.UmvError, match="fp4"):
        ops.gemm(x[:8], _alone(lin), norm_w=torch.ones(1024, dtype=BF16, device="cuda"))
    full = ops.PackedLinear.from_weight_mxfp4(_weights(48, 96, 1).cuda())
    assert full.wp is not None and full.drop_bf16().wp is None
    built = ops.PackedLinear.from_weight_mxfp4(_weights(48, 96, 1).cuda(), keep_bf16=False)
    assert built.wp is None and torch.equal(built.w4, full.w4)
    with pytest.raises(_lib.UmvError, match="MXFP4"):
        ops.PackedLinear.from_weight(_weights(48, 96, 1).cuda()).drop_bf16()


# ----------------------------------------------------------------------------- the engine
FP4_LINEARS = ("qkv", "o", "gate_up", "down")


def _fp4_linears(w):
    return [getattr(lw, f) for part in (w.und, w.gen) for lw in part if lw is not None for f in FP4_LINEARS]


@pytest.fixture(scope="module")
def engines(tiny_weights):
    """(carried, standalone): the same fp4 weights with and without the bf16 images of W'"""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from unimedvl_amd.bagel import Bagel
    from unimedvl_amd.config import UniMedVLConfig
    cfg, sd, _, _ = tiny_weights
    out = []
    for keep in (True, False):
        c = UniMedVLConfig.from_dict(cfg)
        c.llm_weight_dtype = "fp4"
        c.llm_fp4_keep_bf16 = keep
        out.append(Bagel(c, lambda n: sd[n], device="cuda"))
    return out


def _kv_equal(a, b):
    assert a.lens == b.lens
    for sa, sb in zip(a.slabs, b.slabs):
        n = max(a.lens)
        assert torch.equal(sa.k[:, :, :n], sb.k[:, :, :n]) and torch.equal(sa.vt[:, :, :, :n], sb.vt[:, :, :, :n])


def test_standalone_engine_equals_carried_engine(engines, tiny_weights):
    from copy import deepcopy
    from unimedvl_amd.kvcache import NaiveCache
    cfg = tiny_weights[0]
    carried, alone = engines
    wc, wa = carried.language_model.w, alone.language_model.w
    assert wa.fp4 and all(l.wp is None and l.w4 is not None for l in _fp4_linears(wa)) and len(_fp4_linears(wa)) == 8 * cfg["layers"]
    assert all(l.wp is not None for l in _fp4_linears(wc))
    for lc, la in zip(_fp4_linears(wc), _fp4_linears(wa)):
        assert torch.equal(lc.w4, la.w4)
    assert wa.lm_head.w8 is not None and wa.lm_head.wp is not None and wa.lm_head.w4 is None
    g = torch.Generator().manual_seed(11)
    # 3 images of 8 x 8 patches and prompts of 20..38 tokens: both prefill calls run above 64 rows
    imgs = [torch.randn(3, 112, 112, generator=g).clamp(-1, 1) for _ in range(3)]
    prompts = [[int(v) for v in torch.randint(5, 290, (20 + 9 * i,), generator=g)] for i in range(3)]

    class Tok:
        def encode(self, s):
            return prompts[int(s)]

    res = []
    for model in (carried, alone):
        cache = NaiveCache(cfg["layers"])
        gi, kvl, rope = model.prepare_vit_images([0] * 3, [0] * 3, imgs, lambda x: x, NEW_TOKEN_IDS)
        cache = model.forward_cache_update_vit(cache, **gi)
        assert sum(kvl) > 64               # 3 x (8 x 8 patches + 2) rows in one call: the tiled kernel
        gi, kvl, rope = model.prepare_prompts(kvl, rope, ["0", "1", "2"], Tok(), NEW_TOKEN_IDS)
        cache = model.forward_cache_update_text(cache, **gi)
        snap = deepcopy(cache)
        gi = model.prepare_start_tokens(kvl, rope, NEW_TOKEN_IDS)
        ids, logits = model.generate_text(past_key_values=cache, max_length=5, return_logits=True, **gi)
        res.append((snap, ids, logits, kvl, rope))
    assert res[0][3] == res[1][3] and res[0][4] == res[1][4]
    _kv_equal(res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1])
    assert torch.isfinite(res[1][2].float()).all() and torch.equal(res[0][2], res[1][2])


def test_standalone_engine_generate_image_equals_carried(engines, tiny_weights):
    from unimedvl_amd.kvcache import NaiveCache
    cfg = tiny_weights[0]
    prompt = [[int(v) for v in range(7, 40)]]

    class Tok:
        def encode(self, s):
            return prompt[int(s)]

    noise, lats = None, []
    for model in engines:
        gen = NaiveCache(cfg["layers"])
        gi, gkv, grope = model.prepare_prompts([0], [0], ["0"], Tok(), NEW_TOKEN_IDS)
        gen = model.forward_cache_update_text(gen, **gi)
        gi = model.prepare_vae_latent(gkv, grope, [(128, 128)], NEW_TOKEN_IDS)
        if noise is None:
            noise = gi["packed_init_noises"].clone()
        gi["packed_init_noises"] = noise.clone()
        assert noise.shape[0] >= 64           # the flow passes run above 64 rows: the tiled kernel
        lat = model.generate_image(past_key_values=gen, num_timesteps=3, cfg_text_scale=1.0, cfg_img_scale=1.0, timestep_shift=3.0, **gi)
        lats.append(lat[0])
    assert torch.isfinite(lats[0].float()).all() and torch.equal(lats[0], lats[1])


def test_decode_session_96_samples_standalone_equals_carried(engines, tiny_weights, monkeypatch):
    """65..128 samples per step: the split-K branch (6, 8, 8) is the one path where ops.gemm_splitk reaches umv_gemm_mxfp4t"""
    from copy import deepcopy
    from unimedvl_amd import _lib, ops
    from unimedvl_amd.decode import DecodeSession
    from unimedvl_amd.kvcache import NaiveCache
    cfg = tiny_weights[0]
    B = 96
    g = torch.Generator().manual_seed(10)
    prompts = [[int(v) for v in torch.randint(5, 290, (2 + i % 7,), generator=g)] for i in range(B)]

    class Tok:
        def encode(self, s):
            return prompts[int(s)]

    calls = {"t": 0, "w": 0, "b": 0}
    real = ops.gemm_splitk

    def counting(x, lin, partials, k_splits, *, M=None):
        rows = x.shape[0] if M is None else M
        calls["t" if (lin.w4 is not None and lin.wp is None and rows > 64) else "b" if rows > 64 else "w"] += 1
        return real(x, lin, partials, k_splits, M=M)

    monkeypatch.setattr(ops, "gemm_splitk", counting)
    runs = []
    for model in engines:
        cache = NaiveCache(cfg["layers"])
        gi, kvl, rope = model.prepare_prompts([0] * B, [0] * B, [str(i) for i in range(B)], Tok(), NEW_TOKEN_IDS)
        cache = model.forward_cache_update_text(cache, **gi)
        gi = model.prepare_start_tokens(kvl, rope, NEW_TOKEN_IDS)
        before = dict(calls)
        sess = DecodeSession(model.language_model, deepcopy(cache), gi["packed_start_tokens"], gi["packed_query_position_ids"], 5,
                             use_graph=True)
        assert sess.sk == (6, 8, 8)
        lg = []
        for _ in range(4):
            sess.step(1)
            lg.append(sess.logits.float().cpu())
        runs.append((sess.in_ids[:4].cpu(), torch.stack(lg), {k: calls[k] - before[k] for k in calls}))
    assert runs[0][2]["b"] >= 3 * cfg["layers"] and runs[0][2]["t"] == 0, runs[0][2]            # carried: the bf16 image
    assert runs[1][2]["t"] >= 3 * cfg["layers"] and runs[1][2]["b"] == 0, runs[1][2]            # standalone: the MXFP4 image
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert torch.isfinite(runs[1][1]).all()


def test_standalone_mode_frees_the_bf16_images():
    """full width, one LLM layer, both experts: the resident difference is at least the eight dropped images (allocator rounding only adds).
    Measured on MI355X: resident 4 094 284 288 B carried, 3 161 520 640 B standalone, dropped images 932 184 064 B; peak during load
    (not asserted) 6 632 716 288 / 5 700 532 224 B."""
    _ops()
    import gc
    from unimedvl_amd.bagel import Bagel
    from unimedvl_amd.config import UniMedVLConfig
    from unimedvl_amd.weights import random_getter
    dev = torch.device("cuda", 0)
    stats = {}
    dropped = None
    for keep in (True, False):
        gc.collect()
        torch.cuda.empty_cache()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        cfg = UniMedVLConfig(layers=1, vit_layers=1, llm_weight_dtype="fp4", llm_fp4_keep_bf16=keep)
        model = Bagel(cfg, random_getter(cfg, dev, seed=77), device=dev)
        torch.cuda.synchronize()
        stats[keep] = (torch.cuda.memory_allocated() - base, torch.cuda.max_memory_allocated() - base)
        lins = _fp4_linears(model.language_model.w)
        assert len(lins) == 8
        if keep:
            dropped = sum(l.wp.numel() * 2 for l in lins)
        else:
            assert all(l.wp is None for l in lins)
        del model, lins
    print(f"resident carried {stats[True][0]} standalone {stats[False][0]} dropped images {dropped}; "
          f"peak during load carried {stats[True][1]} standalone {stats[False][1]}")
    assert dropped >= 2 * 233_046_016 * 2          # the seven linears of an expert are 233.0 M weights (config.py's dimensions)
    assert stats[True][0] - stats[False][0] >= dropped


def test_inferencer_standalone_fp4_writes_and_hits_its_own_packed_file(tmp_path):
    import json
    import shutil
    from PIL import Image
    from safetensors import safe_open
    from safetensors.torch import save_file
    from conftest import GOLDEN
    from oracle.weights import TINY, make_weights
    from unimedvl_amd.interactive_vqa_inferencer import VQAInferencer
    _ops()
    c = dict(TINY, vocab=704, vit_side=70, max_latent=64)
    sd, _ = make_weights(c, seed=78)
    ckpt = tmp_path / "ckpt"
    ckpt.mkdir()
    json.dump(dict(hidden_size=c["hidden"], num_hidden_layers=c["layers"], num_attention_heads=c["heads"],
                   num_key_value_heads=c["kv_heads"], intermediate_size=c["inter"], vocab_size=c["vocab"], rope_theta=c["rope_theta"],
                   rms_norm_eps=c["rms_eps"], max_position_embeddings=32768), open(ckpt / "llm_config.json", "w"))
    json.dump(dict(hidden_size=c["vit_hidden"], num_hidden_layers=c["vit_layers"] + 1, num_attention_heads=c["vit_heads"],
                   intermediate_size=c["vit_inter"], patch_size=c["patch"]), open(ckpt / "vit_config.json", "w"))
    save_file({k: v.contiguous() for k, v in sd.items()}, str(ckpt / "ema.safetensors"))
    for f in ("vocab.json", "merges.txt", "tokenizer_config.json"):
        shutil.copy(os.path.join(GOLDEN, "tokenizer", f), ckpt / f)
    pil = Image.fromarray(np.random.default_rng(3).integers(0, 255, (300, 420, 3), dtype=np.uint8))
    conf = {"model_path": str(ckpt), "max_new_tokens": 6, "do_sample": False, "llm_weight_dtype": "fp4"}
    q = "What abnormality is visible?"
    vc = VQAInferencer(dict(conf))
    vc.load_model()
    carried_file = ckpt / "ema_packed_w-fp4_a-bf16_und.safetensors"
    assert vc.load_stats["packed_cache"] == "written" and carried_file.exists()
    want = vc.infer_single(pil, q)["answer"]
    conf["llm_fp4_keep_bf16"] = False
    v = VQAInferencer(dict(conf))
    v.load_model()
    own_file = ckpt / "ema_packed_w-fp4_a-bf16-standalone_und.safetensors"
    assert v.load_stats["packed_cache"] == "written" and v.load_stats["from_packed"] == 0 and own_file.exists()
    assert v.infer_single(pil, q)["answer"] == want
    v2 = VQAInferencer(dict(conf))
    v2.load_model()
    assert v2.load_stats["packed_cache"] == "hit" and v2.load_stats["built"] == 0
    w0, w1, w2 = vc.model.language_model.w, v.model.language_model.w, v2.model.language_model.w
    for l0, l1, l2 in zip(w0.und, w1.und, w2.und):
        for f in FP4_LINEARS:
            assert torch.equal(getattr(l0, f).w4, getattr(l2, f).w4) and torch.equal(getattr(l1, f).w4, getattr(l2, f).w4)
            assert getattr(l1, f).wp is None and getattr(l2, f).wp is None and getattr(l0, f).wp is not None
    assert torch.equal(w1.lm_head.w8, w2.lm_head.w8) and w2.lm_head.wp is not None
    assert v2.infer_single(pil, q)["answer"] == want
    with safe_open(str(own_file), framework="pt") as f:
        keys = list(f.keys())
        assert not [k for k in keys if k.startswith("language_model.model.layers") and k.endswith("::wp")]
        assert [k for k in keys if k.startswith("language_model.model.layers") and k.endswith("::w4")]
    assert own_file.stat().st_size < carried_file.stat().st_size
