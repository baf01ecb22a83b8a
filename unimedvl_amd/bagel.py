"""Host-side unified model: the reference's ``Bagel`` inference interface
(codes/modeling/unimedvl/bagel.py:377-1392) over the MI355X engine.

Same method names, argument names and return conventions as the reference, so that
``InterleaveInferencer`` / ``chat``-style callers are drop-ins:
    prepare_prompts / forward_cache_update_text        bagel.py:377 / :412
    prepare_vit_images / forward_cache_update_vit      bagel.py:460 / :523
    prepare_vae_images / forward_cache_update_vae      bagel.py:617 / :697
    prepare_vae_latent / prepare_vae_latent_cfg        bagel.py:809 / :867
    generate_image / _forward_flow                     bagel.py:901 / :989
    prepare_start_tokens / generate_text / chat        bagel.py:1213 / :1236 / :1321
The prepare_* functions build the same packed index tensors on the host (they are the
boundary's data format); the forward_* functions consume what they need of them and
run everything else on the GPU through libunimedvl_hip.so.
"""
from collections import namedtuple
from types import SimpleNamespace
from typing import List, Optional, Tuple

import torch

from . import ops
from .config import UniMedVLConfig
from .data_utils import (PackedVitImages, get_flattened_position_ids_extrapolate, get_flattened_position_ids_interpolate, patchify)
from .decode import DecodeSession
from .sampling import off_neutral, per_sample
from .prep import BagelPrep
from .kvcache import NaiveCache, PagedCache
from .llm import Qwen2MoT
from .vit import SiglipVisionModel
from .weights import GlueWeights, LLMWeights, ViTWeights

# what top_logprobs=n adds to a result (generate_text: tensors [rows, B, n] / [rows, B, n] / [rows, B]; chat: per-token lists)
TopLogprobs = namedtuple("TopLogprobs", ["ids", "logprobs", "rank"])

BF16 = torch.bfloat16


def prefill_score_layout(toks, start, pos0):
    """The rows of Bagel.score_prefill for candidates toks (lists of scored tokens, none empty) behind a context whose start token sits
    at rope position pos0: candidate c with tokens t_0 .. t_{m-1} is the segment [start, t_0, .., t_{m-2}] at positions pos0 .. pos0 + m - 1
    and row i is scored against t_i - the rows and targets `score`'s forced session feeds.  -> (fed ids, targets, query lengths, rope
    positions), the first, second and last one entry per row, candidates back to back."""
    fed, targets, qlens, pos = [], [], [], []
    for t in toks:
        fed += [int(start)] + [int(v) for v in t[:-1]]
        targets += [int(v) for v in t]
        qlens.append(len(t))
        pos += list(range(pos0, pos0 + len(t)))
    return fed, targets, qlens, pos


class Bagel(BagelPrep):
    def __init__(self, cfg: UniMedVLConfig, get, device="cuda", visual_gen=True, visual_und=True,
                 interpolate_pos=False):
        """`get(name)` returns reference-named tensors (see weights.py / shapes.py)."""
        if not torch.cuda.is_available():
            raise RuntimeError("unimedvl_amd needs an MI355X (ROCm) device; there is no CPU fallback")
        BagelPrep.__init__(self, cfg, interpolate_pos)
        self.device = torch.device(device)
        with ops.device_scope(self.device):     # weight packing kernels launch on the current device
            self.language_model = Qwen2MoT(cfg, LLMWeights(cfg, get, self.device, load_gen=visual_gen), self.device)
            self.glue = GlueWeights(cfg, get, self.device, visual_gen, visual_und)
            self.vit_model = SiglipVisionModel(cfg, ViTWeights(cfg, get, self.device), self.device) if visual_und else None
        self.vae_model = None
        self.hidden_size = cfg.hidden
        self.use_moe = True
        self.num_heads = cfg.heads
        self.latent_patch_size = cfg.latent_patch
        self.latent_downsample = cfg.latent_downsample
        self.max_latent_size = cfg.max_latent
        self.latent_channel = cfg.z_channels
        self.patch_latent_dim = cfg.latent_patch ** 2 * cfg.z_channels
        self.vit_patch_size = cfg.patch
        self.vit_max_num_patch_per_side = cfg.vit_side
        self.vit_hidden_size = cfg.vit_hidden
        self.get_flattened_position_ids = (get_flattened_position_ids_interpolate if interpolate_pos
                                           else get_flattened_position_ids_extrapolate)
        self.config = SimpleNamespace(
            llm_config=SimpleNamespace(num_hidden_layers=cfg.layers, hidden_size=cfg.hidden,
                                       num_attention_heads=cfg.heads, layer_module="Qwen2MoTDecoderLayer"),
            visual_gen=visual_gen, visual_und=visual_und, latent_patch_size=cfg.latent_patch,
            max_latent_size=cfg.max_latent, vit_max_num_patch_per_side=cfg.vit_side)
        self.decode_use_graph = True
        self.eos_check_every = 16
        import os
        self.prefill_graph = os.environ.get("UMV_PREFILL_GRAPH", "1") not in ("0", "")   # graph replay of image spans into reserved caches
        # prepare_vit_images hands the engine the transformed images and the patch tokens are made ON THE DEVICE (umv_patchify_f32_bf16);
        # generation_input["packed_vit_tokens"] is then a data_utils.PackedVitImages, which still is the reference's tensor for
        # anyone who asks (UMV_DEVICE_PATCHIFY=0: the reference's host-side permute, 4 ms per 448 x 448 image)
        self.device_patchify = os.environ.get("UMV_DEVICE_PATCHIFY", "1") not in ("0", "")
        self._vit_graphs = {}
        self.prefill_graph_max = 8          # captured image-span graphs kept (one per cache and patch grid; ~0.1 GB of activations each)
        self.beam_context_tokens = 8192     # chat(num_beams > 1): the longest context its paged cache is sized for
        self.chat_cache_tokens = 0          # > 0: chat() prefills / decodes in one pooled, reserved cache of that capacity
        self._chat_cache = None

    def eval(self):
        return self

    # ------------------------------------------------------------------ text
    @torch.no_grad()
    @ops.on_device
    def forward_cache_update_text(self, past_key_values: NaiveCache, packed_text_ids, packed_text_position_ids,
                                  text_token_lens, packed_text_indexes=None, packed_key_value_indexes=None,
                                  key_values_lens=None):
        emb = self.language_model.embed_tokens(packed_text_ids)
        out = self.language_model.forward_inference(
            packed_query_sequence=emb, query_lens=text_token_lens, packed_query_position_ids=packed_text_position_ids,
            packed_query_indexes=packed_text_indexes, past_key_values=past_key_values,
            packed_key_value_indexes=packed_key_value_indexes, key_values_lens=key_values_lens,
            update_past_key_values=True, is_causal=True, mode="und")
        return out.past_key_values

    # ------------------------------------------------------------------ ViT images
    @ops.on_device
    def encode_vit(self, packed_vit_tokens, packed_vit_position_ids, vit_token_seqlens):
        """ViT tower + connector + vit_pos_embed (bagel.py:581-592); returns [N, hidden] bf16 (pre-scatter)."""
        lens = vit_token_seqlens.to("cpu")
        cu = torch.nn.functional.pad(torch.cumsum(lens, dim=0), (1, 0)).to(torch.int32)
        vit = self.vit_model(packed_pixel_values=packed_vit_tokens, packed_flattened_position_ids=packed_vit_position_ids,
                             cu_seqlens=cu, max_seqlen=int(lens.max()))
        h = ops.gemm(vit, self.glue.conn1, act="gelu_tanh")
        return ops.gemm(h, self.glue.conn2)

    # ---- image-span prefill from a HIP graph (profiles/HISTORY.md section 7.4)
    # One 448x448 image is ~460 kernel launches (ViT tower, connector, 28 LLM layers over 1026 tokens): 33 ms of GPU work but
    # ~55 ms of wall time when every launch goes through ctypes.  The shapes depend only on the image's patch grid, and all
    # per-request values (pixels, which cache segment / slot the tokens go to, rope position, keys visible) are read by the
    # kernels from device memory, so for a cache whose slabs stay put (NaiveCache.reserve) the whole span is captured once
    # per (cache, grid) and replayed: the request's pixels and a ~12 KB plan are uploaded, then one graph launch.
    def _vit_graph_key(self, cache, gi):
        if not self.prefill_graph or cache is None or not getattr(cache, "reserved", False) or cache.slabs is None:
            return None
        lens = [int(v) for v in gi["vit_token_seqlens"].tolist()]
        if len(lens) != 1:                       # one image per call (the scripts' and the batcher's admission path)
            return None
        qlens = [int(v) for v in gi["packed_seqlens"].tolist()]
        if max(c + q for c, q in zip(cache.lens, qlens)) > cache.cap:
            return None                          # would re-allocate: the eager path handles (and reports) that
        pos = gi["packed_vit_position_ids"]
        # the captured graph bakes in the K / V^T slab addresses of EVERY layer: all of them are part of the key, so a graph can
        # only be replayed on storage laid out exactly like the one it was captured on (a new cache that happens to reuse the
        # layer-0 address alone must not match - it would be written through stale addresses for the other layers)
        slabs = tuple(p for sl in cache.slabs for p in (sl.k.data_ptr(), sl.vt.data_ptr()))
        # ... and the input kind: a plan made for images (device patchify) cannot be refreshed from a patch tensor or the reverse
        kind = "images" if isinstance(gi["packed_vit_tokens"], PackedVitImages) else "tokens"
        return (slabs, cache.cap, len(cache.lens), lens[0], int(pos[0]), int(pos[-1]), int(gi["packed_text_ids"][0]),
                int(gi["packed_text_ids"][-1]), kind)

    def _vit_graph_run(self, key, cache, gi):
        dev, lm = self.device, self.language_model
        qlens = [int(v) for v in gi["packed_seqlens"].tolist()]
        nseg = len(cache.lens)
        if len(qlens) != nseg:
            raise ValueError(f"cache holds {nseg} samples, call has {len(qlens)}")
        cu = torch.nn.functional.pad(torch.cumsum(gi["vit_token_seqlens"].to("cpu"), dim=0), (1, 0)).to(torch.int32)
        g = self._vit_graphs.get(key)
        if g is None:
            g = SimpleNamespace()
            g.text_ids = gi["packed_text_ids"].to(device=dev, dtype=torch.int64)
            g.text_rows = gi["packed_text_indexes"].to(device=dev, dtype=torch.int32)
            g.vit_rows = gi["packed_vit_token_indexes"].to(device=dev, dtype=torch.int32)
            g.vplan = self.vit_model.make_plan(gi["packed_vit_tokens"], gi["packed_vit_position_ids"], cu, int(gi["vit_token_seqlens"].max()))
            g.lplan = lm.make_plan(qlens, gi["packed_position_ids"], cache.lens)
            g.lplan.max_kv = cache.cap
            T = sum(qlens)

            def body():
                seq = torch.zeros((T, self.hidden_size), dtype=BF16, device=dev)
                lm.embed_tokens(g.text_ids, out=seq, out_rows=g.text_rows)
                vit = self.vit_model(plan=g.vplan)
                conn = ops.gemm(ops.gemm(vit, self.glue.conn1, act="gelu_tanh"), self.glue.conn2)
                ops.add_rows(conn, seq, table=self.glue.vit_pos, idx=g.vplan["pos_ids"], out_rows=g.vit_rows)
                lm.forward_inference(packed_query_sequence=seq, query_lens=g.lplan.qlens, packed_query_position_ids=None,
                                     past_key_values=cache, update_past_key_values=False, is_causal=False, mode="und", plan=g.lplan)
            s = torch.cuda.Stream(device=dev)        # warm-up outside the capture (lazy module loading, allocator)
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                body()
            torch.cuda.current_stream().wait_stream(s)
            g.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g.graph):
                body()
            self._vit_graphs[key] = g
            while len(self._vit_graphs) > self.prefill_graph_max:      # arbitrary image sizes: keep the most recent grids only
                self._vit_graphs.pop(next(iter(self._vit_graphs)))
        else:
            self._vit_graphs[key] = self._vit_graphs.pop(key)          # most recently used last
            self.vit_model.make_plan(gi["packed_vit_tokens"], gi["packed_vit_position_ids"], cu, int(gi["vit_token_seqlens"].max()), into=g.vplan)
            lm.make_plan(qlens, gi["packed_position_ids"], cache.lens, into=g.lplan)
        g.graph.replay()
        cache.lens = [c + q for c, q in zip(cache.lens, qlens)]
        return cache

    @torch.no_grad()
    @ops.on_device
    def forward_cache_update_vit(self, past_key_values: NaiveCache, packed_text_ids, packed_text_indexes,
                                 packed_vit_tokens, packed_vit_token_indexes, packed_vit_position_ids, vit_token_seqlens,
                                 packed_position_ids, packed_seqlens, packed_indexes=None, packed_key_value_indexes=None,
                                 key_values_lens=None):
        dev = self.device
        if key_values_lens is not None and past_key_values is not None and past_key_values.slabs is not None and \
                [int(v) for v in key_values_lens.tolist()] != list(past_key_values.lens):
            raise ValueError(f"key_values_lens {key_values_lens.tolist()} disagree with the cache ({past_key_values.lens})")
        gi = dict(packed_text_ids=packed_text_ids, packed_text_indexes=packed_text_indexes, packed_vit_tokens=packed_vit_tokens,
                  packed_vit_token_indexes=packed_vit_token_indexes, packed_vit_position_ids=packed_vit_position_ids,
                  vit_token_seqlens=vit_token_seqlens, packed_position_ids=packed_position_ids, packed_seqlens=packed_seqlens)
        key = self._vit_graph_key(past_key_values, gi)
        if key is not None:
            return self._vit_graph_run(key, past_key_values, gi)
        T = int(packed_seqlens.sum())
        seq = torch.zeros((T, self.hidden_size), dtype=BF16, device=dev)
        self.language_model.embed_tokens(packed_text_ids, out=seq,
                                         out_rows=packed_text_indexes.to(device=dev, dtype=torch.int32))
        conn = self.encode_vit(packed_vit_tokens, packed_vit_position_ids, vit_token_seqlens)
        ops.add_rows(conn, seq, table=self.glue.vit_pos, idx=packed_vit_position_ids.to(device=dev, dtype=torch.int64),
                     out_rows=packed_vit_token_indexes.to(device=dev, dtype=torch.int32))
        out = self.language_model.forward_inference(
            packed_query_sequence=seq, query_lens=packed_seqlens, packed_query_position_ids=packed_position_ids,
            packed_query_indexes=packed_indexes, past_key_values=past_key_values,
            packed_key_value_indexes=packed_key_value_indexes, key_values_lens=key_values_lens,
            update_past_key_values=True, is_causal=False, mode="und")
        return out.past_key_values

    # ------------------------------------------------------------------ VAE-encoded images (edit / reconstruction)
    @ops.on_device
    def time_embed(self, t_values):
        """TimestepEmbedder (modeling_utils.py:87-109) for a vector of timesteps -> [n, hidden] bf16: the 256-wide sinusoid
        (umv_timestep_embed; the 128 frequencies come from torch once, so t * freqs has the reference's bits), then the two
        linears with the SiLU in the first one's epilogue."""
        import math
        half = 128
        if getattr(self, "_t_freqs", None) is None:
            self._t_freqs = torch.exp(-math.log(10000) * torch.arange(0, half, dtype=torch.float32) / half).to(self.device)
        t = torch.as_tensor(t_values, dtype=torch.float32).reshape(-1).to(self.device)
        emb = ops.timestep_embed(t, self._t_freqs)
        h = ops.gemm(emb, self.glue.time0, act="silu")
        return ops.gemm(h, self.glue.time2)

    @torch.no_grad()
    @ops.on_device
    def forward_cache_update_vae(self, vae_model, past_key_values: NaiveCache, padded_images, patchified_vae_latent_shapes,
                                 packed_vae_position_ids, packed_timesteps, packed_vae_token_indexes, packed_text_ids,
                                 packed_text_indexes, packed_position_ids, packed_seqlens, packed_indexes=None,
                                 key_values_lens=None, packed_key_value_indexes=None, noise=None):
        dev = self.device
        T = int(packed_seqlens.sum())
        seq = torch.zeros((T, self.hidden_size), dtype=BF16, device=dev)
        text_rows = packed_text_indexes.to(device=dev, dtype=torch.int32)
        vae_rows = packed_vae_token_indexes.to(device=dev, dtype=torch.int32)
        self.language_model.embed_tokens(packed_text_ids, out=seq, out_rows=text_rows)
        packed_latent = vae_model.encode_packed(padded_images, patchified_vae_latent_shapes, self.latent_patch_size,
                                                noise=noise)                      # [sum h*w, p*p*c] bf16
        t_emb = self.time_embed(packed_timesteps)                               # [1, hidden]
        x = ops.gemm(packed_latent, self.glue.vae2llm)
        ops.add_rows(x, seq, bcast=t_emb[0], table=self.glue.latent_pos,
                     idx=packed_vae_position_ids.to(device=dev, dtype=torch.int64), out_rows=vae_rows)
        out = self.language_model.forward_inference(
            packed_query_sequence=seq, query_lens=packed_seqlens, packed_query_position_ids=packed_position_ids,
            packed_query_indexes=packed_indexes, past_key_values=past_key_values, key_values_lens=key_values_lens,
            packed_key_value_indexes=packed_key_value_indexes, update_past_key_values=True, is_causal=False, mode="gen",
            packed_vae_token_indexes=packed_vae_token_indexes, packed_text_indexes=packed_text_indexes)
        return out.past_key_values

    # ------------------------------------------------------------------ image generation
    @torch.no_grad()
    @ops.on_device
    def generate_image(self, packed_text_ids, packed_text_indexes, packed_init_noises, packed_vae_position_ids,
                       packed_vae_token_indexes, packed_seqlens, packed_position_ids, packed_indexes=None,
                       past_key_values: NaiveCache = None, key_values_lens=None, packed_key_value_indexes=None,
                       num_timesteps: int = 24, timestep_shift: float = 1.0, cfg_renorm_min: float = 0.0,
                       cfg_renorm_type: str = "global", cfg_interval: Optional[Tuple[float, float]] = (0, 1),
                       cfg_text_scale: float = 1.0, cfg_text_packed_query_indexes=None,
                       cfg_text_packed_position_ids=None, cfg_text_past_key_values: Optional[NaiveCache] = None,
                       cfg_text_key_values_lens=None, cfg_text_packed_key_value_indexes=None,
                       cfg_img_scale: float = 1.0, cfg_img_packed_query_indexes=None, cfg_img_packed_position_ids=None,
                       cfg_img_past_key_values: Optional[NaiveCache] = None, cfg_img_key_values_lens=None,
                       cfg_img_packed_key_value_indexes=None, cfg_type: str = "parallel", callback=None,
                       cfg_renorm_batch_semantics: str = "per_sample"):
        """Rectified-flow Euler sampler with dual CFG + renorm (bagel.py:901-986, 989-1211).

        cfg_renorm_batch_semantics (only matters for cfg_renorm_type="global" with more than one sample in the packed batch):
        "per_sample" (default) takes the renorm norms per sample, i.e. a packed call equals B single-sample calls - the only
        way the reference's inferencer calls this method (inferencer.py:165-232) and what keeps a request's image independent
        of how a batch is sharded over GPUs; "reference" reproduces bagel.py:1196-1198 literally: ONE norm over all the
        latent tokens of the packed batch, which couples the samples."""
        sess = FlowSession(self, locals())
        while not sess.finished:
            sess.step(1)
            if callback is not None:
                callback(sess.i - 1, sess.x_t)
        return sess.latents()

    @staticmethod
    def _contexts_identical(ca, pos_a, cb, pos_b):
        """True only if two KV contexts hold bit-identical keys/values for every layer and the query
        position ids agree (then a forward pass over either gives the same result)."""
        if ca is None or cb is None or pos_a is None or pos_b is None:
            return False
        if ca is cb:
            return torch.equal(pos_a.cpu(), pos_b.cpu())
        if list(ca.lens) == list(cb.lens) and ca.shares_storage_with(cb):     # one is a snapshot of the other: no compare, no sync
            return torch.equal(pos_a.cpu().to(torch.long), pos_b.cpu().to(torch.long))
        if ca.slabs is None or cb.slabs is None or list(ca.lens) != list(cb.lens):
            return False
        if not torch.equal(pos_a.cpu().to(torch.long), pos_b.cpu().to(torch.long)):
            return False
        n = max(ca.lens)
        if n == 0:
            return True
        if min(ca.lens) != n:      # ragged batch: slots past a short sample's length may hold scratch; do not guess
            return False
        diff = torch.zeros((), dtype=torch.int64, device=ca.slabs[0].k.device)
        for sa, sb in zip(ca.slabs, cb.slabs):      # one host sync at the end, not one per layer
            diff += (sa.k[:, :, :n] != sb.k[:, :, :n]).sum() + (sa.vt[:, :, :, :n] != sb.vt[:, :, :, :n]).sum()
        return int(diff.item()) == 0

    # ------------------------------------------------------------------ text generation
    def _sampling_seed(self):
        """Next 62-bit key for the device-side sampler: one draw from the DEVICE's default generator - the generator the
        reference's multinomial consumes (bagel.py:1297-1299 samples on the GPU).  So torch.manual_seed(s) - which reseeds it -
        restarts the stream, also with the same s again (two identical calls each preceded by manual_seed(42) sample identical
        text), successive calls draw new keys, and torch's CPU generator is left untouched (the init noise
        prepare_vae_latent draws afterwards is what it would have been)."""
        return int(torch.randint(0, 2 ** 62, (1,), device=self.device).item())

    @torch.no_grad()
    @ops.on_device
    def generate_text(self, past_key_values: NaiveCache, packed_key_value_indexes=None, key_values_lens=None,
                      packed_start_tokens=None, packed_query_position_ids=None, max_length: int = 0,
                      do_sample: bool = False, temperature: float = 1.0, end_token_id: int = None,
                      return_logits: bool = False, per_sample_eos: bool = False, return_logprobs: bool = False, *,
                      repetition_penalty: float = 1.0, presence_penalty: float = 0.0, frequency_penalty: float = 0.0,
                      logit_bias=None, penalty_context_ids=None, draft_len: int = 0, draft_ngram=(2, 4), draft_context_ids=None,
                      predicted_ids=None, sampling=None, top_logprobs: int = 0, constraint=None, constraint_states=None,
                      no_repeat_ngram_size=0, ngram_context_ids=None, num_beams: int = 1, length_penalty: float = 1.0,
                      early_stopping: bool = False, num_return_sequences: int = 1, bad_words_ids=None, suppress_tokens=None,
                      begin_suppress_tokens=None, min_new_tokens=0, guidance_scale: float = 1.0, guidance_past_key_values=None,
                      guidance_query_position_ids=None, guidance_plausibility: float = 0.0,
                      top_k: int = 0, top_p: float = 1.0, min_p: float = 0.0):
        """Greedy decode (bagel.py:1236-1317).  Returns [steps, B] int64 whose row 0 holds the
        start tokens.  Like the reference, the batch stops when SAMPLE 0 emits end_token_id
        (bagel.py:1313); per_sample_eos=True is the batched extension (stops when every sample
        has emitted it; rows after a sample's EOS keep decoding and should be ignored).
        return_logprobs=True: returns (ids, logprobs) - or (ids, logits, logprobs) with return_logits - where logprobs is fp32
        [rows, B]: logprobs[s] is the log-probability of the token step s picked, ids[s + 1] where that row exists (of
        softmax(logits) in greedy decoding, of softmax(bf16(logits / temperature)) with do_sample).  Needs B <= 64; the step stays
        in the captured graph.
        top_k / top_p / min_p (0 / 1.0 / 0.0 = off; with do_sample): truncated sampling as include/unimedvl_hip.h defines it, in the
        captured step (DecodeSession); B <= 64.  The log-probabilities stay those of the untruncated softmax.
        top_logprobs=n (1..20; implies return_logprobs): one more element at the end of the returned tuple, a TopLogprobs named tuple
        (ids int32 [rows, B, n], logprobs fp32 [rows, B, n], rank int32 [rows, B]): per step the n most likely tokens of the
        untruncated softmax with their log-probabilities, most likely first, and the 1-based rank of the token that was fed; row s
        belongs to ids[s + 1], as for logprobs (include/unimedvl_hip.h, top-n alternative tokens).
        repetition_penalty / presence_penalty / frequency_penalty (1.0 / 0.0 / 0.0 = off) and logit_bias ({token: float}, -inf bans
        a token): the logit penalties of include/unimedvl_hip.h, applied in the captured step before temperature and truncation; ids,
        logits and logprobs are those of the adjusted logits.  penalty_context_ids: per sample a list of tokens (the prompt) that
        count as seen for the repetition penalty - this call has no token ids of its own, so without it that set is empty.
        draft_len > 0: speculative greedy decode (speculative.SpeculativeDecodeSession) - every step verifies draft_len drafted tokens
        per sample, B * (draft_len + 1) <= 64.  The drafts come from predicted_ids (per sample a predicted continuation of the
        generated tokens) where given, else from a lookup of the last draft_ngram = (min, max) tokens in draft_context_ids (per sample
        the prompt's tokens; this call has none of its own) and in what was generated.  Same matrix, same stop rules, same cache
        lengths as draft_len = 0, fewer passes over the weights where drafts are accepted; self.last_draft_stats keeps the session's
        [B, 3] (steps, drafted, accepted).  Greedy only: do_sample, return_logits / return_logprobs, penalties and logit_bias raise.
        sampling (one sampling.SamplingParams, or a list of B): per-request sampling - every sample decodes with its own sampler and
        its own seeded noise (DecodeSession(row_sampling=...); a seed of None is derived from _sampling_seed(), the stream word is the
        sample index).  It excludes the scalar sampler keywords: do_sample, top_k / top_p / min_p, the three penalty keywords and a
        temperature other than 1.0 raise ValueError.  With draft_len > 0 it is sampled speculative decode
        (SpeculativeDecodeSession(sampling=...)): the drafts are verified against each request's own draw, so the matrix is the
        draft_len = 0 matrix (up to the last bit of a logit); return_logprobs is allowed there ([rows, B], aligned as in the plain
        call), while return_logits, top_logprobs, penalised params and logit_bias raise.
        constraint (a constraints.TokenAutomaton) / constraint_states (one start state per sample, default 0, -1 = free): constrained
        decoding in the captured step (DecodeSession) - a sample is only ever fed tokens its automaton state has an edge for; ids,
        logits, logprobs and top_logprobs are those of the masked logits.  With draft_len > 0 it raises.
        no_repeat_ngram_size (n, 0 = off, at most 16; an int or one per sample): no sample is fed a token that would repeat an n-gram
        of its history - HF's NoRepeatNGramLogitsProcessor, in the captured step (DecodeSession; include/unimedvl_hip.h, no-repeat
        n-grams), after the penalties and before the constraint mask; ids, logits, logprobs and top_logprobs are those of the banned
        logits.  The history is the start token and what is fed after it; ngram_context_ids (per sample a token list, the prompt)
        puts tokens in front of that - this call has no token ids of its own.  HF counts the prompt.  With sampling= a sample's size
        is its SamplingParams.no_repeat_ngram_size and the keyword stays 0.  With draft_len > 0 it raises.
        num_beams = K > 1 (at most 10, B * K <= 64): beam search decode (beam.BeamDecodeSession; include/unimedvl_hip.h, beam search
        decode) as HF's generate(num_beams=K, do_sample=False) defines it, with length_penalty and early_stopping (True / False) as
        there.  past_key_values must be a PagedCache (ValueError otherwise): the beams decode on a throwaway fork that shares the
        prompt's pages, and the cache itself is left as it was - nothing is committed to it.  Returns the usual matrix holding every
        sample's BEST hypothesis: row 0 the start tokens, then its tokens, the end token included; rows after a sample's end token
        are filled with the end token.  return_logprobs=True adds fp32 [rows - 1, B]: row s the log-probability of ids[s + 1] (0
        behind a sample's end).  self.last_beam_hypotheses keeps, per sample, the num_return_sequences (<= K) best hypotheses as
        dicts (tokens, tokens_no_end, score - the length-normalised one -, total, logprobs).  Excludes do_sample, sampling,
        draft_len, top_logprobs, return_logits, constraint, the penalties, logit_bias, no_repeat_ngram_size and top_k / top_p /
        min_p (ValueError before any launch); 1 = off: today's call.
        bad_words_ids (token lists of at most 16), suppress_tokens, begin_suppress_tokens (token lists) and min_new_tokens (an int or
        one per sample; bans end_token_id, which it needs): HF's keywords of these names, in the captured step (DecodeSession;
        include/unimedvl_hip.h, banned sequences) behind the n-gram ban and before the constraint mask; ids, logits, logprobs and
        top_logprobs are those of the banned logits.  The history is the start token and what is fed after it: a bad word that begins
        in the prompt is not seen.  They are the one logit stage that also runs with num_beams > 1 (every beam by its own tokens).
        With draft_len > 0 they raise.
        guidance_scale = g != 1 (finite, >= 0): classifier-free guidance for text - HF's guidance_scale
        (UnbatchedClassifierFreeGuidanceLogitsProcessor), in the captured step (guidance.GuidedDecodeSession; include/unimedvl_hip.h,
        classifier-free guidance for text).  guidance_past_key_values: the unconditional contexts, a second NaiveCache with the same
        number of segments (the prompt without its images - visual contrastive decoding -, or a negative prompt);
        guidance_query_position_ids: their rope positions.  Every step the logits become g * (log_softmax(cond) -
        log_softmax(uncond)) + log_softmax(uncond), before temperature and truncation; ids, logprobs and top_logprobs are those of the
        guided distribution.  guidance_plausibility = beta in [0, 1): tokens whose conditional probability is below beta times the
        most likely token's are dropped first (the adaptive plausibility constraint of contrastive decoding; 0 = HF exactly).  The
        call decodes on a merged copy of the two caches (2 B <= 64 rows) and leaves BOTH as they were - nothing is committed.  Slab
        caches only.  Combines with do_sample / temperature, top_k / top_p / min_p, return_logprobs, top_logprobs and
        per_sample_eos; everything else (ops.GUIDANCE_EXCLUDES: beams, drafts, sampling=, penalties, logit_bias, bans, constraint,
        return_logits) raises ValueError before any launch.  1.0 = off: today's call."""
        guidance_scale, guidance_plausibility = ops.check_guidance(
            guidance_scale, guidance_plausibility, num_beams=num_beams, draft_len=draft_len, sampling=sampling,
            repetition_penalty=repetition_penalty, presence_penalty=presence_penalty, frequency_penalty=frequency_penalty,
            logit_bias=logit_bias, no_repeat_ngram_size=no_repeat_ngram_size, constraint=constraint, bad_words_ids=bad_words_ids,
            suppress_tokens=suppress_tokens, begin_suppress_tokens=begin_suppress_tokens, min_new_tokens=min_new_tokens,
            return_logits=return_logits)
        if guidance_scale != 1.0:
            return self._generate_text_guided(past_key_values, key_values_lens, packed_start_tokens, packed_query_position_ids, max_length,
                                              end_token_id, per_sample_eos, return_logprobs, top_logprobs, guidance_scale,
                                              guidance_past_key_values, guidance_query_position_ids, guidance_plausibility,
                                              dict(do_sample=do_sample, temperature=temperature, top_k=top_k, top_p=top_p, min_p=min_p))
        if guidance_past_key_values is not None or guidance_query_position_ids is not None:
            raise ValueError("guidance_past_key_values / guidance_query_position_ids go with guidance_scale != 1")
        num_beams = ops.check_beams(num_beams, self.cfg.vocab, len(past_key_values.lens))
        words, suppress, begin, mins, _ = ops.check_sequences(bad_words_ids, suppress_tokens, begin_suppress_tokens, min_new_tokens,
                                                              end_token_id if min_new_tokens else None, vocab=self.cfg.vocab,
                                                              rows=len(past_key_values.lens))
        banned = {}                          # what is on, under DecodeSession's names
        if words or suppress or begin:
            banned.update(bad_words_ids=words, suppress_tokens=suppress, begin_suppress_tokens=begin)
        if any(mins) if isinstance(mins, list) else mins:
            banned.update(min_new_tokens=mins)
        if banned and draft_len:
            raise ValueError("bad_words_ids / suppress_tokens / begin_suppress_tokens / min_new_tokens are not available with "
                             "draft_len > 0 (speculative decode)")
        if num_beams > 1:
            from .beam import check_beam_keywords
            check_beam_keywords(num_beams, do_sample=do_sample, sampling=sampling, draft_len=draft_len, top_logprobs=top_logprobs,
                                return_logits=return_logits, constraint=constraint, repetition_penalty=repetition_penalty,
                                presence_penalty=presence_penalty, frequency_penalty=frequency_penalty, logit_bias=logit_bias,
                                no_repeat_ngram_size=no_repeat_ngram_size, top_k=top_k, top_p=top_p, min_p=min_p)
            return self._generate_text_beams(past_key_values, packed_start_tokens, packed_query_position_ids, max_length, end_token_id,
                                             return_logprobs, num_beams, length_penalty, early_stopping, num_return_sequences, banned)
        if "min_new_tokens" in banned:
            banned.update(end_token_id=end_token_id)
        sizes = [ops.check_ngram(v) for v in no_repeat_ngram_size] if isinstance(no_repeat_ngram_size, (list, tuple)) else \
            [ops.check_ngram(no_repeat_ngram_size)]
        if draft_len and (any(sizes) or (sampling is not None and any(p.no_repeat_ngram_size for p in per_sample(
                sampling, len(past_key_values.lens))))):
            raise ValueError("no_repeat_ngram_size is not available with draft_len > 0 (speculative decode)")
        if constraint is None and constraint_states is not None:
            raise ValueError("constraint_states goes with constraint")
        if constraint is not None and draft_len:
            raise ValueError("constraint is not available with draft_len > 0 (speculative decode)")
        if sampling is not None:
            scalar = off_neutral(locals())
            if scalar:
                raise ValueError(f"sampling excludes the scalar sampler keywords (got {scalar})")
            sampling = per_sample(sampling, len(past_key_values.lens))
        top_k, top_p, min_p = ops.check_truncation(top_k, top_p, min_p)
        top_logprobs = ops.check_top_logprobs(top_logprobs, self.cfg.vocab)
        return_logprobs = bool(return_logprobs) or top_logprobs > 0
        ops.check_penalties(repetition_penalty, presence_penalty, frequency_penalty, logit_bias, vocab=self.cfg.vocab)
        # do_sample: softmax(logits / temperature) + multinomial on the device (bagel.py:1297-1299).  The
        # draw is keyed by a seed derived from torch.initial_seed(), so torch.manual_seed(s) makes runs
        # reproducible; the stream itself is not torch's (no device can reproduce another's RNG).
        seed = self._sampling_seed() if do_sample or (sampling and any(p.do_sample and p.seed is None for p in sampling)) else 0
        if key_values_lens is not None and [int(v) for v in key_values_lens.tolist()] != list(past_key_values.lens):
            raise ValueError("key_values_lens disagree with the cache")
        if max_length <= 0:   # nothing to decode (the reference would fail on torch.stack([]) here, bagel.py:1316)
            out = torch.zeros((0, len(past_key_values.lens)), dtype=torch.int64, device=self.device)
            res = (out,)
            if return_logits:
                res += (torch.zeros((0, len(past_key_values.lens), self.cfg.vocab), dtype=BF16, device=self.device),)
            if return_logprobs:
                res += (torch.zeros((0, len(past_key_values.lens)), dtype=torch.float32, device=self.device),)
            if top_logprobs:
                shape = (0, len(past_key_values.lens), top_logprobs)
                res += (TopLogprobs(torch.zeros(shape, dtype=torch.int32, device=self.device),
                                    torch.zeros(shape, dtype=torch.float32, device=self.device),
                                    torch.zeros(shape[:2], dtype=torch.int32, device=self.device)),)
            return res if len(res) > 1 else out
        if draft_len and sampling is not None:
            if return_logits or top_logprobs:
                raise ValueError("sampled speculative decode (draft_len > 0 with sampling) has no return_logits / top_logprobs")
            if logit_bias:
                raise ValueError("sampled speculative decode (draft_len > 0 with sampling) takes no logit_bias")
            return self._generate_text_speculative(past_key_values, packed_start_tokens, packed_query_position_ids, max_length,
                                                   end_token_id, per_sample_eos, draft_len, draft_ngram, draft_context_ids, predicted_ids,
                                                   dict(sampling=sampling, seed=seed, logprobs=return_logprobs))
        if draft_len:
            if return_logits or return_logprobs:
                raise ValueError("speculative decode (draft_len > 0) is greedy only: no return_logits / return_logprobs / top_logprobs")
            return self._generate_text_speculative(past_key_values, packed_start_tokens, packed_query_position_ids, max_length,
                                                   end_token_id, per_sample_eos, draft_len, draft_ngram, draft_context_ids, predicted_ids,
                                                   dict(do_sample=do_sample, top_k=top_k, top_p=top_p, min_p=min_p,
                                                        repetition_penalty=repetition_penalty, presence_penalty=presence_penalty,
                                                        frequency_penalty=frequency_penalty, logit_bias=logit_bias,
                                                        penalty_context_ids=penalty_context_ids))
        sampler = dict(do_sample=do_sample, temperature=temperature, top_k=top_k, top_p=top_p, min_p=min_p,
                       repetition_penalty=repetition_penalty, presence_penalty=presence_penalty, frequency_penalty=frequency_penalty)
        if sampling is not None:             # every sample its own sampler and key; the stream word is the sample index
            sampler = dict(row_sampling=sampling)
        sess = DecodeSession(self.language_model, past_key_values, packed_start_tokens, packed_query_position_ids,
                             max_length, use_graph=self.decode_use_graph and not return_logits, seed=seed, logprobs=return_logprobs,
                             logit_bias=logit_bias, penalty_context_ids=penalty_context_ids, top_logprobs=top_logprobs,
                             constraint=constraint, constraint_states=constraint_states, no_repeat_ngram_size=no_repeat_ngram_size,
                             ngram_context_ids=ngram_context_ids, **banned, **sampler)
        logits = []
        steps = 0
        stop = None
        while steps < max_length:
            n = 1 if return_logits else min(self.eos_check_every, max_length - steps)
            sess.step(n)
            if return_logits:
                logits.append(sess.logits.clone())
            steps += n
            if end_token_id is not None:
                pred = sess.pred_ids[:steps].cpu()
                hit = pred == end_token_id
                if per_sample_eos:
                    if bool(hit.any(0).all()):
                        stop = int(hit.float().argmax(0).max()) + 1
                        break
                elif bool(hit[:, 0].any()):
                    stop = int(hit[:, 0].float().argmax()) + 1
                    break
        rows = stop if stop is not None else steps
        sess.commit(rows)
        out = sess.in_ids[:rows].clone()
        res = (out,)
        if return_logits:
            res += (torch.stack(logits[:rows], 0),)
        if return_logprobs:
            res += (sess.pred_logprobs[:rows].clone(),)
        if top_logprobs:
            res += (TopLogprobs(sess.pred_top_ids[:rows].clone(), sess.pred_top_logprobs[:rows].clone(), sess.pred_rank[:rows].clone()),)
        return res if len(res) > 1 else out

    def _generate_text_guided(self, cache, key_values_lens, start_tokens, positions, max_length, end_token_id, per_sample_eos,
                              return_logprobs, top_logprobs, scale, uncond, uncond_positions, beta, sampler):
        """generate_text with guidance_scale != 1: one guided decode on a merged copy of `cache` and `uncond`, the conditional rows as
        the usual matrix.  Both caches are read, never written."""
        from .guidance import GuidedDecodeSession
        if hasattr(cache, "ensure_tokens") or hasattr(uncond, "ensure_tokens"):
            raise ValueError("guidance_scale != 1 decodes on slab caches (NaiveCache): a PagedCache is not available")
        if uncond is None or uncond_positions is None:
            raise ValueError("guidance_scale != 1 needs guidance_past_key_values and guidance_query_position_ids (the unconditional contexts)")
        B = len(cache.lens)
        if len(uncond.lens) != B or uncond.slabs is None or cache.slabs is None:
            raise ValueError(f"guidance_past_key_values must hold the same number of prefilled segments as past_key_values ({B}), "
                             f"got {len(uncond.lens)}")
        if 2 * B > 64:
            raise ValueError(f"guidance_scale != 1 decodes two rows per sample: at most 32 samples, got {B}")
        if key_values_lens is not None and [int(v) for v in key_values_lens.tolist()] != list(cache.lens):
            raise ValueError("key_values_lens disagree with the cache")
        sampler["top_k"], sampler["top_p"], sampler["min_p"] = ops.check_truncation(sampler["top_k"], sampler["top_p"], sampler["min_p"])
        top_logprobs = ops.check_top_logprobs(top_logprobs, self.cfg.vocab)
        return_logprobs = bool(return_logprobs) or top_logprobs > 0
        if max_length <= 0:
            out = torch.zeros((0, B), dtype=torch.int64, device=self.device)
            res = (out,)
            if return_logprobs:
                res += (torch.zeros((0, B), dtype=torch.float32, device=self.device),)
            if top_logprobs:
                shape = (0, B, top_logprobs)
                res += (TopLogprobs(torch.zeros(shape, dtype=torch.int32, device=self.device),
                                    torch.zeros(shape, dtype=torch.float32, device=self.device),
                                    torch.zeros(shape[:2], dtype=torch.int32, device=self.device)),)
            return res if len(res) > 1 else out
        seed = self._sampling_seed() if sampler["do_sample"] else 0
        cfg = self.cfg
        both = NaiveCache.merged([cache, uncond], [B, B], max_length + 1, cfg.kv_heads, cfg.head_dim, self.device)
        sess = GuidedDecodeSession(self.language_model, both, start_tokens, positions, max_length, scale,
                                   guidance_positions=uncond_positions, guidance_plausibility=beta, use_graph=self.decode_use_graph,
                                   seed=seed, logprobs=return_logprobs, top_logprobs=top_logprobs, **sampler)
        steps, stop = 0, None
        while steps < max_length:
            n = min(self.eos_check_every, max_length - steps)
            sess.step(n)
            steps += n
            if end_token_id is not None:
                hit = sess.tokens(steps).cpu() == end_token_id
                if per_sample_eos:
                    if bool(hit.any(0).all()):
                        stop = int(hit.float().argmax(0).max()) + 1
                        break
                elif bool(hit[:, 0].any()):
                    stop = int(hit[:, 0].float().argmax()) + 1
                    break
        rows = stop if stop is not None else steps
        self.last_guidance_lse = sess.lse.clone()
        out = sess.fed(rows).clone()
        res = (out,)
        if return_logprobs:
            res += (sess.token_logprobs(rows).clone(),)
        if top_logprobs:
            res += (TopLogprobs(*(t.clone() for t in sess.top(rows))),)
        return res if len(res) > 1 else out

    def _generate_text_beams(self, cache, start_tokens, positions, max_length, end_token_id, return_logprobs, num_beams, length_penalty,
                             early_stopping, num_return_sequences, banned=None):
        """generate_text with num_beams > 1: one beam search on a fork of `cache`, the best hypotheses as the usual matrix.  banned:
        the banned-sequence keywords that are on (beam_generate's names)"""
        from .beam import beam_generate, check_beam_options
        check_beam_options(num_beams, length_penalty, early_stopping, num_return_sequences)
        if not hasattr(cache, "fork_beams"):
            raise ValueError(f"num_beams > 1 needs past_key_values to be a PagedCache, got {type(cache).__name__}")
        B = len(cache.lens)
        starts = start_tokens.to(device=self.device, dtype=torch.int64).reshape(1, -1)
        if max_length <= 0:
            self.last_beam_hypotheses = [[] for _ in range(B)]
            out = torch.zeros((0, B), dtype=torch.int64, device=self.device)
            return (out, torch.zeros((0, B), dtype=torch.float32, device=self.device)) if return_logprobs else out
        hyps = beam_generate(self.language_model, cache, start_tokens, positions, max_length, num_beams, end_token_id=end_token_id,
                             length_penalty=length_penalty, early_stopping=early_stopping, num_return_sequences=num_return_sequences,
                             use_graph=self.decode_use_graph, eos_check_every=self.eos_check_every, **(banned or {}))
        self.last_beam_hypotheses = hyps
        n = max(len(h[0]["tokens"]) for h in hyps)
        fill = 0 if end_token_id is None else int(end_token_id)
        ids = torch.full((n, B), fill, dtype=torch.int64)
        lps = torch.zeros((n, B), dtype=torch.float32)
        for b, h in enumerate(hyps):
            ids[:len(h[0]["tokens"]), b] = torch.tensor(h[0]["tokens"], dtype=torch.int64)
            lps[:len(h[0]["logprobs"]), b] = torch.tensor(h[0]["logprobs"], dtype=torch.float32)
        out = torch.cat([starts, ids.to(self.device)], 0)
        return (out, lps.to(self.device)) if return_logprobs else out

    def _generate_text_speculative(self, cache, start_tokens, positions, max_length, end_token_id, per_sample_eos, draft_len,
                                   draft_ngram, draft_context_ids, predicted_ids, plain):
        """generate_text with drafts: the plain call's matrix row s + 1 is a sample's emitted token s.  The plain call stops at row
        `stop` - sample 0's first end token, or the last of every sample's first - and returns that many rows, leaving as many tokens
        in the cache; here a sample may be ahead of another, so when the stop row is known every sample's limit is lowered to it and
        the steps go on until each holds that many tokens."""
        from .speculative import SpeculativeDecodeSession
        sess = SpeculativeDecodeSession(self.language_model, cache, start_tokens, positions, max_length, draft_len,
                                        use_graph=self.decode_use_graph, draft_ngram=draft_ngram, draft_context_ids=draft_context_ids,
                                        predicted_ids=predicted_ids, **plain)
        stop = None
        while True:
            sess.step(min(self.eos_check_every, max_length - sess.steps_done))
            n_out = sess.n_out.cpu()
            if end_token_id is not None and stop is None:
                out = sess.out_ids.cpu()
                first = []                       # per sample the row after its first end token, None while it has emitted none
                for b in range(out.shape[0]):
                    hit = (out[b, :int(n_out[b])] == end_token_id).nonzero()
                    first.append(int(hit[0]) + 1 if hit.numel() else None)
                if per_sample_eos:
                    stop = max(first) if all(f is not None for f in first) else None
                else:
                    stop = first[0]
                if stop is not None:
                    sess.limit.fill_(stop)
            rows = stop if stop is not None else max_length
            if int(n_out.min()) >= rows or sess.steps_done >= max_length:
                break
        sess.commit(rows)
        self.last_draft_stats = sess.stats.cpu()
        out = torch.cat([start_tokens.to(device=self.device, dtype=torch.int64).reshape(1, -1), sess.out_ids[:, :rows - 1].t()], 0)
        if sess.out_logprobs is not None:        # row s: the log-probability of emitted token s = out[s + 1], as the plain call has it
            return out, sess.out_logprobs[:, :rows].t().contiguous()
        return out

    # ------------------------------------------------------------------ convenience (evaluation path)
    @torch.no_grad()
    @ops.on_device
    def chat(self, tokenizer, new_token_ids, image_transform, images, prompt, max_length: int,
             do_sample: bool = False, temperature: float = 1.0, return_logprobs: bool = False, *,
             repetition_penalty: float = 1.0, presence_penalty: float = 0.0, frequency_penalty: float = 0.0, logit_bias=None,
             penalize_prompt: bool = False, draft_len: int = 0, draft_ngram=(2, 4), predicted_ids=None,
             sampling=None, top_logprobs: int = 0, choices=None, choices_after: str = "stop",
             no_repeat_ngram_size: int = 0, no_repeat_ngram_prompt: bool = False,
             num_beams: int = 1, length_penalty: float = 1.0, early_stopping: bool = False, num_return_sequences: int = 1,
             bad_words_ids=None, bad_words=None, suppress_tokens=None, begin_suppress_tokens=None, min_new_tokens: int = 0,
             guidance_scale: float = 1.0, negative_prompt=None, guidance_plausibility: float = 0.0,
             top_k: int = 0, top_p: float = 1.0, min_p: float = 0.0):
        """ViT-only VQA convenience path (bagel.py:1321-1392).  return_logprobs=True: returns (answer, token_ids, token_logprobs) -
        the generated tokens behind the answer (the end token excluded) and the log-probability of each (generate_text).
        top_logprobs=n (implies return_logprobs): a fourth element, a TopLogprobs named tuple of per-token lists - ids and logprobs
        (n entries per token, most likely first) and rank (the token's own 1-based rank).
        repetition_penalty / presence_penalty / frequency_penalty / logit_bias: the logit penalties of generate_text;
        penalize_prompt=True makes the prompt's token ids the repetition penalty's context set (off: generated tokens only) - the
        text's own tokens, not the bos / eos wrapper around them: a penalised end token would only make answers longer.
        draft_len > 0: speculative greedy decode (generate_text) - the same answer from fewer passes over the weights where the answer
        repeats the prompt's wording or its own; the prompt's text tokens are the lookup's context.  predicted_ids: a predicted answer
        (a string, or its token ids) to draft from instead.
        sampling (a sampling.SamplingParams): the request's own sampler and seed instead of the scalar sampler keywords
        (generate_text) - with draft_len > 0 sampled speculative decode, the same answer as with draft_len = 0.
        choices (strings, tokenised as `score` tokenises its candidates, or lists of token ids): guided choice - the answer is one of
        them (constraints.TokenAutomaton.from_choices; generate_text(constraint=)), picked by the sampler the other keywords set, the
        end token after it.  choices_after="free": the answer STARTS with one of them and goes on as free text.  `score` ranks a closed
        set exactly at one forced row per candidate; choices costs one row, samples, and returns the sampler's pick.
        no_repeat_ngram_size (0 = off): the answer repeats no n-gram of that size (generate_text); with sampling= the size is the
        SamplingParams'.  no_repeat_ngram_prompt=True seeds the history with the prompt's text tokens - the list penalize_prompt
        uses, without the bos / eos wrapper - so that an n-gram of the prompt is not repeated either; the default counts generated
        tokens only.  (HF's generate counts the prompt.)
        num_beams > 1: beam search decode (generate_text) - the context is prefilled into a PagedCache of its own
        (self.beam_context_tokens bounds the prompt) and the best hypothesis is the answer; length_penalty / early_stopping as HF's.
        With num_return_sequences > 1 the call returns a list of (answer, score), best first.  It excludes what generate_text
        excludes, and `choices`.
        bad_words_ids / suppress_tokens / begin_suppress_tokens / min_new_tokens: generate_text's (HF's) keywords - phrases and tokens
        the answer must not hold, and the number of tokens it holds at the least before the end token may come; also with num_beams.
        bad_words (strings): each is encoded twice, bare and with a leading space - a word inside a sentence and one at its start
        are different tokens - and both token sequences join bad_words_ids (ops.encode_bad_words); a phrase is banned as the
        tokenizer splits it, other spellings (capitals, no space after a bracket) are other phrases.
        guidance_scale != 1: classifier-free guidance for text (generate_text) - the answer is decoded from the contrast of the
        context above with an UNCONDITIONAL context prefilled into a cache of its own: negative_prompt (a string) as its only text,
        or - negative_prompt=None - the same prompt with its images dropped (visual contrastive decoding: what the answer owes to
        the language prior alone is pushed down).  Without images and without a negative_prompt there is nothing to contrast:
        ValueError.  guidance_plausibility: generate_text's.  It excludes what generate_text excludes, and `choices`."""
        guidance_scale, guidance_plausibility = ops.check_guidance(
            guidance_scale, guidance_plausibility, num_beams=num_beams, draft_len=draft_len, sampling=sampling, choices=choices,
            repetition_penalty=repetition_penalty, presence_penalty=presence_penalty, frequency_penalty=frequency_penalty,
            logit_bias=logit_bias, no_repeat_ngram_size=no_repeat_ngram_size, bad_words_ids=bad_words_ids, bad_words=bad_words,
            suppress_tokens=suppress_tokens, begin_suppress_tokens=begin_suppress_tokens, min_new_tokens=min_new_tokens)
        if guidance_scale == 1.0 and negative_prompt is not None:
            raise ValueError("negative_prompt goes with guidance_scale != 1")
        if guidance_scale != 1.0 and negative_prompt is None and not images:
            raise ValueError("guidance_scale != 1 without images and without a negative_prompt: there is nothing to contrast")
        if num_beams > 1:
            from .beam import check_beam_keywords
            check_beam_keywords(ops.check_beams(num_beams, self.cfg.vocab, 1), choices=choices, draft_len=draft_len, sampling=sampling)
        constraint = None
        if choices is not None:
            from .constraints import TokenAutomaton
            constraint = TokenAutomaton.from_choices([tokenizer.encode(c) if isinstance(c, str) else [int(v) for v in c] for c in choices],
                                                     int(new_token_ids["eos_token_id"]), after=choices_after)
        if num_beams > 1:                    # the beams fork the prompt's pages: pages for the context, and two per beam and page index
            P = ops.KV_PAGE
            private = 2 * num_beams * ((max_length + 1 + P - 1) // P + 1)
            cache = PagedCache(self.cfg.layers, pool_pages=(self.beam_context_tokens + P - 1) // P + private + 1,
                               max_context=self.beam_context_tokens + max_length + 1 + P)
        elif self.chat_cache_tokens > 0:       # serving: one reserved cache reused by every request (stable slabs -> graph prefill)
            if self._chat_cache is None or self._chat_cache.cap < self.chat_cache_tokens:
                self._chat_cache = NaiveCache(self.cfg.layers)
                self._chat_cache.reserve(1, self.chat_cache_tokens, self.cfg.kv_heads, self.cfg.head_dim, self.device)
            cache = self._chat_cache
            cache.lens = [0]
        else:
            cache = NaiveCache(self.cfg.layers)
        newlens, new_rope = [0], [0]
        for image in images:
            gi, newlens, new_rope = self.prepare_vit_images(newlens, new_rope, [image], image_transform, new_token_ids)
            cache = self.forward_cache_update_vit(cache, **gi)
        gi, newlens, new_rope = self.prepare_prompts(newlens, new_rope, [prompt], tokenizer, new_token_ids)
        text_ids = gi["packed_text_ids"].tolist()[1:-1]                                          # without the bos / eos wrapper
        prompt_ids = [text_ids] if penalize_prompt else None
        draft = {}
        if draft_len:
            if isinstance(predicted_ids, str):
                predicted_ids = tokenizer.encode(predicted_ids)
            draft = dict(draft_len=draft_len, draft_ngram=draft_ngram, draft_context_ids=[text_ids],
                         predicted_ids=None if predicted_ids is None else [list(predicted_ids)])
        cache = self.forward_cache_update_text(cache, **gi)
        gi = self.prepare_start_tokens(newlens, new_rope, new_token_ids)
        guided = {}
        if guidance_scale != 1.0:            # the unconditional context: a text-only prefill into a cache of its own
            ulens, urope = [0], [0]
            ugi, ulens, urope = self.prepare_prompts(ulens, urope, [prompt if negative_prompt is None else negative_prompt], tokenizer,
                                                     new_token_ids)
            ucache = self.forward_cache_update_text(NaiveCache(self.cfg.layers), **ugi)
            guided = dict(guidance_scale=guidance_scale, guidance_plausibility=guidance_plausibility, guidance_past_key_values=ucache,
                          guidance_query_position_ids=self.prepare_start_tokens(ulens, urope, new_token_ids)["packed_query_position_ids"])
        ids = self.generate_text(past_key_values=cache, max_length=max_length, do_sample=do_sample, **guided,
                                 temperature=temperature, end_token_id=new_token_ids["eos_token_id"],
                                 return_logprobs=return_logprobs, top_k=top_k, top_p=top_p, min_p=min_p, top_logprobs=top_logprobs,
                                 repetition_penalty=repetition_penalty, presence_penalty=presence_penalty,
                                 frequency_penalty=frequency_penalty, logit_bias=logit_bias, penalty_context_ids=prompt_ids,
                                 sampling=sampling, constraint=constraint, no_repeat_ngram_size=no_repeat_ngram_size,
                                 ngram_context_ids=[text_ids] if no_repeat_ngram_prompt else None, num_beams=num_beams,
                                 length_penalty=length_penalty, early_stopping=early_stopping, num_return_sequences=num_return_sequences,
                                 bad_words_ids=list(bad_words_ids or []) + ops.encode_bad_words(tokenizer, bad_words),
                                 suppress_tokens=suppress_tokens, begin_suppress_tokens=begin_suppress_tokens,
                                 min_new_tokens=min_new_tokens, **draft, **gi)
        if num_beams > 1 and num_return_sequences > 1:
            def text(tokens):
                return tokenizer.decode(torch.tensor([int(gi["packed_start_tokens"][0])] + tokens)).split("<|im_end|>")[0].split("<|im_start|>")[1]
            return [(text(h["tokens"]), h["score"]) for h in self.last_beam_hypotheses[0]]
        top = None
        if top_logprobs:
            ids, lp, top = ids
        elif return_logprobs:
            ids, lp = ids
        output = tokenizer.decode(ids[:, 0].cpu())
        answer = output.split("<|im_end|>")[0].split("<|im_start|>")[1]
        if num_beams > 1 and return_logprobs:           # the best hypothesis' own lists, the end token excluded
            best = self.last_beam_hypotheses[0][0]
            return answer, best["tokens_no_end"], best["logprobs"][:len(best["tokens_no_end"])]
        if return_logprobs or top is not None:          # lp[s] belongs to ids[s + 1]
            n = max(ids.shape[0] - 1, 0)
            res = (answer, ids[1:, 0].tolist(), lp[:n, 0].tolist())
            if top is not None:
                res += (TopLogprobs(top.ids[:n, 0].tolist(), top.logprobs[:n, 0].tolist(), top.rank[:n, 0].tolist()),)
            return res
        return answer

    @torch.no_grad()
    @ops.on_device
    def score(self, tokenizer, new_token_ids, image_transform, images, prompt, candidates, append_eos: bool = True):
        """Closed-set answering: how probable is each candidate answer after the context of `chat` (images, then the prompt)?
        candidates: strings (tokenizer.encode) or lists of token ids, at most 64.  The context is prefilled ONCE, laid out once
        per candidate (NaiveCache.merged) and one forced decode session feeds every candidate its own tokens - append_eos adds the
        end token, so that "yes" is not favoured over "yes, but" for being a prefix - with -1 (free-running, ignored) past a
        candidate's end.  Greedy definition: log-softmax of the bf16 logits.  Returns one dict per candidate: token_ids (the scored
        tokens, EOS included), token_logprobs (one fp32 value per token) and logprob (their sum, added in fp64 on the host).
        Samples are independent rows of every kernel, so a candidate's values do not depend on the others.
        Forced decoding costs one decode step per token - the right trade for answers of a few tokens; long continuations want the
        prefill-time scorer, score_prefill: the same rows and targets in one forward pass.  score_top_logprobs adds every token's rank
        and alternatives."""
        return self._score(tokenizer, new_token_ids, image_transform, images, prompt, candidates, append_eos, None)

    @torch.no_grad()
    @ops.on_device
    def score_prefill(self, tokenizer, new_token_ids, image_transform, images, prompt, candidates, append_eos: bool = True, *,
                      rows_per_pass: int = 1024, fused: bool = True):
        """`score` for long candidates - report sentences, long multiple-choice options, the perplexity of a reference text, beam
        hypotheses to re-rank: the rows `score`'s forced session feeds one step at a time - per candidate the segment [start, t_0, ..,
        t_{m-2}] at consecutive slots and rope positions behind the context, row i scored against t_i - run through ONE prefill pass
        over a NaiveCache.merged copy of the context per candidate, and Qwen2MoT.token_logprobs turns the returned rows into
        log-probabilities without storing logits (rows_per_pass rows of lm_head per launch over one reused workspace; fused=False:
        the unfused composition over stored logits - what an e4m3 lm_head takes either way).  Same candidates (1..64), same dict per
        candidate (token_ids, token_logprobs, logprob = the fp64 host sum) and same ValueErrors as `score`, plus one for a candidate
        that would pass max_position.  The values are the prefill kernels': they agree with `score`'s to the kernels' tolerance, not
        bit for bit.  Ranks and top-n alternatives stay with score_top_logprobs.  The context cache is left as it was."""
        toks = self._score_candidates(tokenizer, new_token_ids, candidates, append_eos)
        cache, gi = self._score_context(tokenizer, new_token_ids, image_transform, images, prompt)
        cfg, lm, n = self.cfg, self.language_model, len(toks)
        fed, targets, qlens, pos = prefill_score_layout(toks, int(gi["packed_start_tokens"][0]), int(gi["packed_query_position_ids"][0]))
        if max(pos) >= cfg.max_position:
            raise ValueError(f"score_prefill: the longest candidate ({max(qlens)} tokens) would pass max_position ({cfg.max_position}): "
                             f"its last row sits at rope position {max(pos)}")
        if min(targets) < 0 or max(targets) >= cfg.vocab:
            raise ValueError(f"score_prefill: candidate tokens must lie in the vocabulary [0, {cfg.vocab})")
        many = NaiveCache.merged([cache] * n, [1] * n, max(qlens) + 1, cfg.kv_heads, cfg.head_dim, self.device)
        out = lm.forward_inference(packed_query_sequence=lm.embed_tokens(torch.tensor(fed, dtype=torch.int64)), query_lens=qlens,
                                   packed_query_position_ids=torch.tensor(pos, dtype=torch.int32), past_key_values=many,
                                   update_past_key_values=False, is_causal=True, mode="und")
        lp = lm.token_logprobs(out.packed_query_sequence, torch.tensor(targets, dtype=torch.int64), rows_per_pass, fused=fused).cpu()
        res, r0 = [], 0
        for t in toks:
            vals = lp[r0:r0 + len(t)]
            res.append({"token_ids": t, "token_logprobs": vals.tolist(), "logprob": float(vals.double().sum())})
            r0 += len(t)
        return res

    @torch.no_grad()
    @ops.on_device
    def score_top_logprobs(self, tokenizer, new_token_ids, image_transform, images, prompt, candidates, append_eos: bool = True,
                           top_logprobs: int = 0):
        """`score` whose dicts also carry token_ranks - per token its 1-based rank among the vocabulary at its step ("was the right
        answer's token in the top 5?") - and, with top_logprobs = n > 0 (at most 20), top_logprobs: per token a list of n (id, logprob)
        pairs, most likely first (include/unimedvl_hip.h, top-n alternative tokens).  The other entries are `score`'s own bits.
        (n = 0 still costs a one-alternative launch per step: the rank comes from the same kernel.)  A method of its own because
        `score`'s parameter list is pinned."""
        return self._score(tokenizer, new_token_ids, image_transform, images, prompt, candidates, append_eos, top_logprobs)

    @staticmethod
    def _score_candidates(tokenizer, new_token_ids, candidates, append_eos):
        """the scored tokens of every candidate of score / score_prefill: strings through tokenizer.encode, the end token behind them"""
        cands = list(candidates)
        if not 1 <= len(cands) <= 64:
            raise ValueError(f"score takes 1..64 candidates, got {len(cands)}")
        toks = []
        for c in cands:
            t = [int(v) for v in (tokenizer.encode(c) if isinstance(c, str) else c)]
            if append_eos:
                t.append(int(new_token_ids["eos_token_id"]))
            if not t:
                raise ValueError("score: an empty candidate (and append_eos=False) has nothing to score")
            toks.append(t)
        return toks

    def _score_context(self, tokenizer, new_token_ids, image_transform, images, prompt):
        """the context of `chat` (images, then the prompt) prefilled once -> (its cache, the start tokens behind it)"""
        cache = NaiveCache(self.cfg.layers)
        newlens, new_rope = [0], [0]
        for image in images:
            gi, newlens, new_rope = self.prepare_vit_images(newlens, new_rope, [image], image_transform, new_token_ids)
            cache = self.forward_cache_update_vit(cache, **gi)
        gi, newlens, new_rope = self.prepare_prompts(newlens, new_rope, [prompt], tokenizer, new_token_ids)
        cache = self.forward_cache_update_text(cache, **gi)
        return cache, self.prepare_start_tokens(newlens, new_rope, new_token_ids)

    def _score(self, tokenizer, new_token_ids, image_transform, images, prompt, candidates, append_eos, top_logprobs):
        ranks = top_logprobs is not None
        want_top = ops.check_top_logprobs(top_logprobs, self.cfg.vocab) if ranks else 0
        toks = self._score_candidates(tokenizer, new_token_ids, candidates, append_eos)
        cfg, n, steps = self.cfg, len(toks), max(len(t) for t in toks)
        cache, gi = self._score_context(tokenizer, new_token_ids, image_transform, images, prompt)
        many = NaiveCache.merged([cache] * n, [1] * n, steps + 1, cfg.kv_heads, cfg.head_dim, self.device) if n > 1 else cache
        forced = torch.full((steps, n), -1, dtype=torch.int64)
        for b, t in enumerate(toks):
            forced[:len(t), b] = torch.tensor(t, dtype=torch.int64)
        sess = DecodeSession(self.language_model, many, gi["packed_start_tokens"].repeat(n), gi["packed_query_position_ids"].repeat(n),
                             steps, use_graph=self.decode_use_graph, forced_ids=forced, top_logprobs=max(want_top, 1) if ranks else 0)
        sess.step(steps)
        lp = sess.pred_logprobs.cpu()
        if ranks:
            rk, tid, tlp = sess.pred_rank.cpu(), sess.pred_top_ids.cpu(), sess.pred_top_logprobs.cpu()
        out = []
        for b, t in enumerate(toks):
            vals = lp[:len(t), b]
            out.append({"token_ids": t, "token_logprobs": vals.tolist(), "logprob": float(vals.double().sum())})
            if ranks:
                out[-1]["token_ranks"] = rk[:len(t), b].tolist()
            if want_top:
                out[-1]["top_logprobs"] = [list(zip(tid[s, b, :want_top].tolist(), tlp[s, b, :want_top].tolist())) for s in range(len(t))]
        return out


class FlowSession:
    """The rectified-flow sampler of Bagel.generate_image (bagel.py:901-986, 989-1211) as a RESUMABLE object: the setup of
    generate_image, then `step(n)` = n Euler steps.  generate_image runs it to the end; the mixed VQA + T2I scheduler
    (serving.MixedBatcher, BASELINE.json configs[4]) interleaves its steps with the decode steps of the VQA slots."""

    def __init__(self, model, a):
        m = self.m = model
        packed_text_ids, packed_text_indexes = a["packed_text_ids"], a["packed_text_indexes"]
        packed_init_noises, packed_vae_position_ids = a["packed_init_noises"], a["packed_vae_position_ids"]
        packed_vae_token_indexes, packed_seqlens, packed_position_ids = a["packed_vae_token_indexes"], a["packed_seqlens"], a["packed_position_ids"]
        past_key_values, key_values_lens = a["past_key_values"], a["key_values_lens"]
        num_timesteps, timestep_shift = a["num_timesteps"], a["timestep_shift"]
        cfg_renorm_type, cfg_text_scale, cfg_img_scale = a["cfg_renorm_type"], a["cfg_text_scale"], a["cfg_img_scale"]
        cfg_text_past_key_values, cfg_text_packed_position_ids = a["cfg_text_past_key_values"], a["cfg_text_packed_position_ids"]
        cfg_img_past_key_values, cfg_img_packed_position_ids = a["cfg_img_past_key_values"], a["cfg_img_packed_position_ids"]
        self.cfg_interval, self.cfg_renorm_min = a["cfg_interval"], a["cfg_renorm_min"]
        self.cfg_text_scale, self.cfg_img_scale = cfg_text_scale, cfg_img_scale
        batch_sem = a.get("cfg_renorm_batch_semantics", "per_sample")
        if batch_sem not in ("per_sample", "reference"):
            raise ValueError(f"cfg_renorm_batch_semantics must be 'per_sample' or 'reference', got {batch_sem!r}")
        self._setup(model, packed_text_ids, packed_text_indexes, packed_init_noises, packed_vae_position_ids,
                           packed_vae_token_indexes, packed_seqlens, packed_position_ids, past_key_values, key_values_lens,
                           num_timesteps, timestep_shift, cfg_renorm_type, cfg_text_scale, cfg_text_past_key_values,
                           cfg_text_packed_position_ids, cfg_img_scale, cfg_img_past_key_values, cfg_img_packed_position_ids, batch_sem)

    def _setup(self, m, packed_text_ids, packed_text_indexes, packed_init_noises, packed_vae_position_ids,
               packed_vae_token_indexes, packed_seqlens, packed_position_ids, past_key_values, key_values_lens,
               num_timesteps, timestep_shift, cfg_renorm_type, cfg_text_scale, cfg_text_past_key_values,
               cfg_text_packed_position_ids, cfg_img_scale, cfg_img_past_key_values, cfg_img_packed_position_ids, batch_sem):
        s = self     # (m = the Bagel model; the body below is generate_image's former setup)
        if cfg_renorm_type not in ("global", "channel", "text_channel"):
            raise NotImplementedError(f"{cfg_renorm_type} is not suppoprted")
        dev = m.device
        lm, g = m.language_model, m.glue
        x_t = packed_init_noises.to(device=dev, dtype=torch.float32).contiguous().clone()
        N, D = x_t.shape
        seqlens = [int(v) for v in packed_seqlens.tolist()]
        T = sum(seqlens)
        # schedule on the host in fp32, exactly as the reference builds it (bagel.py:937-940)
        ts = torch.linspace(1, 0, num_timesteps)
        ts = timestep_shift * ts / (1 + (timestep_shift - 1) * ts)
        dts = ts[:-1] - ts[1:]
        ts = ts[:-1]
        t_emb_all = m.time_embed(ts)                           # rows identical within a step: compute once
        text_rows = packed_text_indexes.to(device=dev, dtype=torch.int32)
        vae_rows = packed_vae_token_indexes.to(device=dev, dtype=torch.int32)
        vae_pos = packed_vae_position_ids.to(device=dev, dtype=torch.int64)
        seg_off = [0]
        for n in seqlens:
            seg_off.append(seg_off[-1] + n - 2)
        seg_off_d = torch.tensor(seg_off, dtype=torch.int32).to(dev)
        # The reference runs the conditional, no-text and no-image passes one after another
        # (bagel.py:1120-1171).  They share the query tokens and the weights and differ only in their KV
        # context, and samples are independent, so here they are ONE packed forward over nctx*B segments
        # of a merged cache: the weights stream once instead of three times and the GEMMs see 3x the rows.
        B = len(seqlens)
        use_text = cfg_text_scale > 1.0
        use_img = use_text and cfg_img_scale > 1.0   # the reference computes the image pass but drops it when
        ctxs = [(past_key_values, packed_position_ids)]                      # cfg_text_scale <= 1 (bagel.py:1173,1208)
        if use_text:
            ctxs.append((cfg_text_past_key_values, cfg_text_packed_position_ids))
        # Pure text-to-image: the "no image" context holds exactly the tokens of the conditional one
        # (inferencer.py:587,602), so its velocity equals v_t bit for bit (same rows through the same
        # deterministic kernels).  When the two caches and position ids are PROVABLY identical the third pass
        # is skipped and v_img := v_t; the CFG arithmetic is unchanged.
        img_same = use_img and m._contexts_identical(past_key_values, packed_position_ids,
                                                        cfg_img_past_key_values, cfg_img_packed_position_ids)
        if use_img and not img_same:
            ctxs.append((cfg_img_past_key_values, cfg_img_packed_position_ids))
        nctx = len(ctxs)
        cfgm = m.cfg
        for c, _ in ctxs:
            if c is None:
                raise ValueError("classifier-free guidance needs the cfg_* contexts")
        if key_values_lens is not None and past_key_values.slabs is not None and \
                [int(v) for v in key_values_lens.tolist()] != list(past_key_values.lens):
            raise ValueError("key_values_lens disagree with the cache")
        if nctx > 1:
            merged = NaiveCache.merged([c for c, _ in ctxs], [B] * nctx, max(seqlens), cfgm.kv_heads, cfgm.head_dim, dev)
            base = merged.view_segments(0, B)
        else:
            merged = base = past_key_values
        seq_all = torch.zeros((nctx * T, m.hidden_size), dtype=BF16, device=dev)
        rows_text = torch.cat([text_rows + c * T for c in range(nctx)])
        rows_vae = torch.cat([vae_rows + c * T for c in range(nctx)])
        lm.embed_tokens(packed_text_ids.repeat(nctx), out=seq_all, out_rows=rows_text)
        pos_all = torch.cat([p.to(torch.long).cpu() for _, p in ctxs])
        seqlens_all = torch.tensor(seqlens * nctx, dtype=torch.int)
        seq1 = seq_all[:T]

        def forward(n, cache):
            out = lm.forward_inference(
                packed_query_sequence=seq_all[:n * T], query_lens=seqlens_all[:n * B],
                packed_query_position_ids=pos_all[:n * T], past_key_values=cache, update_past_key_values=False,
                is_causal=False, mode="gen", packed_vae_token_indexes=rows_vae[:n * N], packed_text_indexes=rows_text[:n * 2 * B])
            return ops.gemm(out.packed_query_sequence, g.llm2vae)          # [n*T, D]; vae rows picked by the CFG kernel

        s.rtype = {"global": 0, "channel": 1, "text_channel": 2}[cfg_renorm_type]
        if batch_sem == "reference" and s.rtype == 0 and B > 1:
            # bagel.py:1196-1198: ONE norm over every latent token of the packed batch
            seg_off_d = torch.tensor([0, N], dtype=torch.int32).to(dev)
            s.renorm_segments = 1
        else:
            s.renorm_segments = B
        s.x_t, s.D, s.T, s.N, s.B, s.nctx = x_t, D, T, N, B, nctx
        s.ts, s.dts, s.t_emb_all = ts, dts, t_emb_all
        s.use_text, s.use_img, s.img_same = use_text, use_img, img_same
        s.seq_all, s.vae_pos, s.vae_rows, s.seg_off_d = seq_all, vae_pos, vae_rows, seg_off_d
        s.merged, s.base, s.forward, s.seqlens = merged, base, forward, seqlens
        s.i = 0
        return s

    @property
    def finished(self):
        return self.i >= len(self.ts)

    @property
    def steps_left(self):
        return len(self.ts) - self.i

    @torch.no_grad()
    def step(self, n=1):
        """n Euler steps (fewer if the schedule ends)."""
        s, m = self, self.m
        g = m.glue
        with ops.device_scope(m.device):
            for _ in range(n):
                if s.finished:
                    return
                i = s.i
                t = float(s.ts[i])
                guided = s.use_text and t > s.cfg_interval[0] and t <= s.cfg_interval[1]
                s_text, s_img = (s.cfg_text_scale, s.cfg_img_scale) if guided else (1.0, 1.0)
                xb = ops.cast_pad(s.x_t, s.D)
                h = ops.gemm(xb, g.vae2llm)
                T = s.T
                for c in range(s.nctx if guided else 1):
                    ops.add_rows(h, s.seq_all[c * T:(c + 1) * T], bcast=s.t_emb_all[i], table=g.latent_pos, idx=s.vae_pos, out_rows=s.vae_rows)
                if guided:
                    v = s.forward(s.nctx, s.merged)
                    v_t, v_text = v[:T], v[T:2 * T]
                    v_img = (v_t if s.img_same else v[2 * T:3 * T]) if s.use_img else None
                else:
                    v_t, v_text, v_img = s.forward(1, s.base), None, None
                ops.cfg_renorm_euler(s.x_t, v_t, v_text, v_img, s.vae_rows, s.seg_off_d, s.renorm_segments, s_text,
                                     s_img if s.use_img else 1.0, s.cfg_renorm_min, s.rtype, float(s.dts[i]))
                s.i += 1

    def latents(self):
        return self.x_t.split([n - 2 for n in self.seqlens])
