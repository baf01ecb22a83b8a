"""MXFP4 weight path (llm_weight_dtype = "fp4") on the GPU, through the C ABI:
  * umv_quantize_pack_weight_mxfp4 == tests/mxfp4_ref.py bit for bit (codes, block scales, W', and the bf16 image of W');
  * every code survives v_cvt_scalef32_pk_bf16_fp4 at every kind of scale;
  * umv_gemm_mxfp4w == umv_gemm_bf16 on W', bit for bit (K % 512 == 0, no split-K: same K slices, same MFMAs);
  * the engine with llm_weight_dtype="fp4" against the CPU oracle run on W', at the fp8 path's tolerances;
  * serving and the packed-file fast path with fp4 weights."""
import functools
import os

import numpy as np
import pytest
import torch

from conftest import NEW_TOKEN_IDS
from mxfp4_ref import dequantised_weights_mxfp4, quantize, unpack_image

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def _ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from unimedvl_amd import ops
    return ops


def _weights(N, K, seed):
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(N, K, generator=g) * torch.exp(torch.randn(N, 1, generator=g) * 2) * 0.02).to(BF16)
    w[1] = 0                                          # all-zero blocks
    w[2, :32] = -w[2, :32].abs() * 2.0 ** -126        # bf16 subnormals: the e = -127 clamp, negative values rounding to -0
    w[3, 32:64] = 2.0 ** -128
    w[4, :16] = 6.0 * 2.0 ** torch.arange(16)         # amax exactly 6 * 2^e
    return w


@pytest.mark.parametrize("N,K", [(48, 512), (100, 96), (200, 1056), (16, 32)])
def test_quantize_pack_matches_restatement(N, K):
    ops = _ops()
    w = _weights(N, K, N * 7 + K)
    lin = ops.PackedLinear.from_weight_mxfp4(w.cuda())
    codes, e8, deq = quantize(w)
    c, s = unpack_image(lin.w4, N, K)
    assert torch.equal(c, codes) and torch.equal(s, e8)
    # the bf16 image carried for M > 64 is the packed image of exactly W' (-0 included)
    ref = ops.PackedLinear.from_weight(deq.cuda())
    assert torch.equal(lin.wp.cpu().view(torch.int16), ref.wp.cpu().view(torch.int16))


def test_quantize_pack_swiglu_matches_restatement():
    ops = _ops()
    I, K = 48, 160
    gate, up = _weights(I, K, 5), _weights(I, K, 6) * 3
    lin = ops.PackedLinear.from_gate_up_mxfp4(gate.cuda(), up.cuda())
    (cg, cu), (sg, su) = unpack_image(lin.w4, 2 * I, K, swiglu_I=I)
    qg, qu = quantize(gate), quantize(up)
    assert torch.equal(cg, qg[0]) and torch.equal(sg, qg[1]) and torch.equal(cu, qu[0]) and torch.equal(su, qu[1])
    ref = ops.PackedLinear.from_gate_up(qg[2].cuda(), qu[2].cuda())
    assert torch.equal(lin.wp.cpu().view(torch.int16), ref.wp.cpu().view(torch.int16))


def test_every_code_survives_the_device_conversion():
    """x = one-hot rows: out[m, n] = W'[n, m] exactly, for all 16 codes at scales from 2^-127 to 2^100."""
    ops = _ops()
    from mxfp4_ref import CODE_VALUES
    K, N = 64, 48
    g = torch.Generator().manual_seed(3)
    codes = torch.randint(0, 16, (N, K), generator=g)
    codes[:, :16] = torch.arange(16)
    codes[:, 32:48] = torch.arange(16)
    e = torch.tensor([-127, -126, -100, -3, 0, 5, 60, 100])[torch.arange(N * 2) % 8].view(N, 2)
    w = (CODE_VALUES[codes] * torch.pow(2.0, e.double()).repeat_interleave(32, dim=1)).to(BF16)
    lin = ops.PackedLinear.from_weight_mxfp4(w.cuda())
    deq = quantize(w)[2]
    x = torch.eye(K, dtype=BF16, device="cuda")
    out = ops.gemm(x, lin)
    assert torch.equal(out.cpu(), deq.t().contiguous())
    assert deq.abs().min() == 0 and (deq != 0).sum() > N * K // 2


@functools.lru_cache(maxsize=None)
def _lin(N, K, swiglu):
    ops = _ops()
    g = torch.Generator(device="cuda").manual_seed(N + K)
    if swiglu:
        gate = (torch.randn(N // 2, K, device="cuda", generator=g) * 0.02).to(BF16)
        up = (torch.randn(N // 2, K, device="cuda", generator=g) * 0.02).to(BF16)
        return ops.PackedLinear.from_gate_up_mxfp4(gate, up)
    w = (torch.randn(N, K, device="cuda", generator=g) * 0.02).to(BF16)
    b = (torch.randn(N, device="cuda", generator=g) * 0.1).to(BF16)
    return ops.PackedLinear.from_weight_mxfp4(w, b)


def _bf16_twin(lin):
    ops = _ops()
    return ops.PackedLinear(lin.wp, lin.bias, lin.N, lin.K, swiglu=lin.swiglu)


@pytest.mark.parametrize("M", [1, 8, 16, 17, 40, 64])
@pytest.mark.parametrize("N,K,swiglu", [(4608, 3584, False), (3584, 3584, False), (2 * 18944, 3584, True), (3584, 18944, False),
                                        (200, 1024, False)])
def test_gemm_bit_identical_to_bf16_on_dequantised_weights(M, N, K, swiglu):
    ops = _ops()
    lin = _lin(N, K, swiglu)
    g = torch.Generator(device="cuda").manual_seed(M)
    x = torch.randn(M, K, device="cuda", generator=g).to(BF16)
    out = ops.gemm(x, lin)
    ref = ops.gemm(x, _bf16_twin(lin))
    assert torch.isfinite(out.float()).all()
    if swiglu and M > 32:       # umv_gemm_bf16 runs a tiled kernel here (whole K per workgroup): same products, another fp32 order
        assert torch.allclose(out.float(), ref.float(), rtol=2 ** -6, atol=1e-3)
    else:
        assert torch.equal(out, ref)


def test_gemm_epilogues_and_row_idx():
    ops = _ops()
    lin = _lin(4608, 3584, False)
    twin = _bf16_twin(lin)
    g = torch.Generator(device="cuda").manual_seed(9)
    x = torch.randn(20, 3584, device="cuda", generator=g).to(BF16)
    res = torch.randn(20, 4608, device="cuda", generator=g).to(BF16)
    idx = torch.tensor([19, 3, 7, 0, 11, 12, 5, 2], dtype=torch.int32, device="cuda")
    outs = []
    for l in (lin, twin):
        o = res.clone()
        ops.gemm(x, l, out=o, M=8, residual=o, row_idx=idx)
        f = ops.gemm(x[:8], l, out_f32=True, use_bias=False)
        outs.append((o, f))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    untouched = torch.ones(20, dtype=torch.bool)
    untouched[idx.cpu().long()] = False
    assert torch.equal(outs[0][0][untouched.cuda()], res[untouched.cuda()])


def test_gemm_k_not_a_multiple_of_512():
    # other K partition than the bf16 kernel: same products, fp32 sums in another order
    ops = _ops()
    lin = _lin(320, 96 * 11, False)
    x = torch.randn(8, 96 * 11, device="cuda").to(BF16)
    out = ops.gemm(x, lin, out_f32=True)
    ref = ops.gemm(x, _bf16_twin(lin), out_f32=True)
    assert (out - ref).abs().max() <= 1e-4 * ref.abs().max()


def _seq_sum(p):
    acc = p[0].clone()
    for s in range(1, p.shape[0]):
        acc += p[s]
    return acc


@pytest.mark.parametrize("M", [8, 32, 64])
@pytest.mark.parametrize("N,K,S", [(4608, 3584, 3), (3584, 18944, 4), (320, 1024, 3)])
def test_splitk_partials(M, N, K, S):
    ops = _ops()
    lin = _lin(N, K, False)
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(M + S)).to(BF16).cuda()
    p = torch.full((S, M, N), float("nan"), dtype=torch.float32, device="cuda")
    ops.gemm_splitk(x, lin, p, S)
    p16 = torch.empty_like(p)
    ops.gemm_splitk(x, ops.PackedLinear(lin.wp, None, lin.N, lin.K), p16, S)
    scale = _seq_sum(p16).abs().max().clamp_min(1e-3)
    assert torch.isfinite(p).all() and (_seq_sum(p) - _seq_sum(p16)).abs().max() <= 1e-3 * scale


def test_gemm_argument_rejection():
    import ctypes as C
    from unimedvl_amd import _lib
    ops = _ops()
    lib = _lib.load()
    lin = _lin(200, 1024, False)
    x = torch.randn(80, 1024, device="cuda").to(BF16)
    out = torch.empty(80, 200, dtype=BF16, device="cuda")

    def call(**kw):
        a = dict(x=x.data_ptr(), ldx=1024, wp=lin.w4.data_ptr(), out=out.data_ptr(), ldo=200, M=8, N=200, K=1024, epilogue=0)
        a.update(kw)
        return _lib.check(lib.umv_gemm_mxfp4w(C.byref(_lib.GemmArgs(**a)), ops._stream()), "umv_gemm_mxfp4w")

    call()
    with pytest.raises(_lib.UmvError, match="M <= 64"):
        call(M=65)
    with pytest.raises(_lib.UmvError, match="multiple of 32"):
        call(K=1000)
    with pytest.raises(_lib.UmvError, match="w_scale must be NULL"):
        call(w_scale=out.data_ptr())
    amax = torch.zeros(8, 13, dtype=torch.int64, device="cuda")
    with pytest.raises(_lib.UmvError, match="argmax_partial"):
        call(argmax_partial=amax.data_ptr())
    with pytest.raises(_lib.UmvError, match="multiple of 32"):
        ops.PackedLinear.from_weight_mxfp4(torch.zeros(16, 48, dtype=BF16, device="cuda"))
    # above 64 rows ops.gemm takes the bf16 image of W' on the tiled kernel
    assert torch.equal(ops.gemm(x, lin), ops.gemm(x, _bf16_twin(lin)))


# ----------------------------------------------------------------------------- the engine
@pytest.fixture(scope="module")
def engine_fp4(tiny_weights):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from unimedvl_amd.bagel import Bagel
    from unimedvl_amd.config import UniMedVLConfig
    cfg, sd, _, _ = tiny_weights
    c = UniMedVLConfig.from_dict(cfg)
    c.llm_weight_dtype = "fp4"
    return Bagel(c, lambda n: sd[n], device="cuda")


def test_engine_fp4_vqa_matches_oracle_on_dequantised_weights(engine_fp4, tiny_weights):
    from oracle.unimedvl_cpu import OracleBagel, KVCache
    from unimedvl_amd.kvcache import NaiveCache
    cfg, sd, vae_sd, _ = tiny_weights
    model = engine_fp4
    w = model.language_model.w
    assert w.fp4 and not w.fp8 and w.und[0].qkv.w4 is not None and w.gen[0].down.w4 is not None
    assert w.lm_head.w8 is not None and w.lm_head.w4 is None
    assert w.decode_weight_bytes() == w.lm_head.w8.numel() + sum(l.w4.numel() for lw in w.und for l in (lw.qkv, lw.o, lw.gate_up, lw.down))
    g = torch.Generator().manual_seed(11)
    imgs = [torch.randn(3, 42, 56, generator=g).clamp(-1, 1), torch.randn(3, 28, 70, generator=g).clamp(-1, 1)]
    prompts = [[11, 22, 33, 44], [55, 66, 77]]

    class Tok:
        def encode(self, s):
            return prompts[int(s)]

    cache = NaiveCache(cfg["layers"])
    gi, kvl, rope = model.prepare_vit_images([0, 0], [0, 0], imgs, lambda x: x, NEW_TOKEN_IDS)
    cache = model.forward_cache_update_vit(cache, **gi)
    gi, kvl, rope = model.prepare_prompts(kvl, rope, ["0", "1"], Tok(), NEW_TOKEN_IDS)
    cache = model.forward_cache_update_text(cache, **gi)
    gi = model.prepare_start_tokens(kvl, rope, NEW_TOKEN_IDS)
    ids, logits = model.generate_text(past_key_values=cache, max_length=5, return_logits=True, **gi)

    o = OracleBagel(cfg, dequantised_weights_mxfp4(sd), vae_sd, attn_impl="sdpa")
    oc = KVCache(cfg["layers"], 2)
    okv, orope = o.update_vit(oc, [0, 0], [0, 0], imgs, NEW_TOKEN_IDS)
    bos, eos = NEW_TOKEN_IDS["bos_token_id"], NEW_TOKEN_IDS["eos_token_id"]
    okv, orope = o.update_text(oc, okv, orope, [[bos] + p + [eos] for p in prompts])
    oids, ologits = o.generate_text(oc, orope, bos, 5, return_logits=True)
    assert okv == kvl and orope == rope
    lg, rl = logits.float().cpu(), ologits.float()
    for s in range(5):
        assert torch.equal(ids[s].cpu(), oids[s]), f"fed token differs at step {s}"
        d = (lg[s] - rl[s]).abs().max().item()
        assert d <= 0.25, f"logits differ by {d} at step {s}"
        cos = torch.nn.functional.cosine_similarity(lg[s].flatten(), rl[s].flatten(), dim=0).item()
        assert cos > 0.999
        top2 = rl[s].topk(2, dim=-1).values
        sure = (top2[:, 0] - top2[:, 1]) > 0.25
        assert torch.equal(lg[s].argmax(-1)[sure], rl[s].argmax(-1)[sure])
        if not torch.equal(lg[s].argmax(-1), rl[s].argmax(-1)):
            break
    # quantisation is not a no-op: the bf16 oracle's logits differ visibly from the fp4 model's
    o16 = OracleBagel(cfg, sd, vae_sd, attn_impl="sdpa")
    oc16 = KVCache(cfg["layers"], 2)
    k16, r16 = o16.update_vit(oc16, [0, 0], [0, 0], imgs, NEW_TOKEN_IDS)
    k16, r16 = o16.update_text(oc16, k16, r16, [[bos] + p + [eos] for p in prompts])
    _, l16 = o16.generate_text(oc16, r16, bos, 1, return_logits=True)
    assert (l16[0].float() - rl[0]).abs().max().item() > 1e-3


def test_paged_batcher_with_fp4_weights_matches_single_requests(engine_fp4):
    from oracle.toy_tokenizer import ToyTokenizer
    from unimedvl_amd.serving import ContinuousBatcher
    tok = ToyTokenizer(NEW_TOKEN_IDS)
    g = torch.Generator().manual_seed(21)
    reqs = [([torch.randn(3, 28, 42, generator=g).clamp(-1, 1)] if i % 2 else [],
             " ".join(str(int(v)) for v in torch.randint(5, 290, (2 + i,), generator=g))) for i in range(5)]
    budgets = [6, 3, 5, 6, 2]
    ident = lambda x: x   # noqa: E731
    want = [engine_fp4.chat(tok, NEW_TOKEN_IDS, ident, im, pr, max_length=nb + 1) for (im, pr), nb in zip(reqs, budgets)]
    srv = ContinuousBatcher(engine_fp4, tok, NEW_TOKEN_IDS, ident, slots=3, max_context=256, max_new_tokens=8, check_every=3,
                            paged=True, pool_pages=16)
    rids = [srv.submit(im, pr, max_new_tokens=nb) for (im, pr), nb in zip(reqs, budgets)]
    got = srv.run()
    assert [got[r] for r in rids] == want


def test_inferencer_fp4_writes_and_hits_its_packed_file(tmp_path):
    import json
    import shutil
    from PIL import Image
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
    v = VQAInferencer(dict(conf))
    v.load_model()
    assert v.load_stats["packed_cache"] == "written" and (ckpt / "ema_packed_w-fp4_a-bf16_und.safetensors").exists()
    a = v.infer_single(pil, "What abnormality is visible?")["answer"]
    v2 = VQAInferencer(dict(conf))
    v2.load_model()
    assert v2.load_stats["packed_cache"] == "hit" and v2.load_stats["built"] == 0
    w1, w2 = v.model.language_model.w, v2.model.language_model.w
    assert w2.fp4 and w2.und[0].qkv.w4 is not None
    for l1, l2 in zip(w1.und, w2.und):
        for f in ("qkv", "o", "gate_up", "down"):
            assert torch.equal(getattr(l1, f).w4, getattr(l2, f).w4)
    assert torch.equal(w1.lm_head.w8, w2.lm_head.w8)
    assert v2.infer_single(pil, "What abnormality is visible?")["answer"] == a
