"""VQA entry point - importable counterpart of the reference's notebook-style script
(codes/interactive_vqa_inferencer.py:58-336): same ``DEFAULT_CONFIG`` keys, same
``VQAInferencer(config).load_model()`` / ``.infer_single(image_path, prompt, temperature,
max_new_tokens, do_sample, show_image)`` returning the same result dict.  Keys that only
steered accelerate's CPU staging (enable_cpu_loading, offload_folder, max_mem_per_gpu,
enable_auto_bf16_conversion) are accepted and ignored: weights stream from the
memory-mapped safetensors file to the GPU tensor by tensor.
"""
import gc
import os
import time
from datetime import datetime
from typing import Any, Dict, Optional

import torch
from PIL import Image

from .bagel import Bagel
from . import packstore
from .checkpoint import checkpoint_getter, checkpoint_source_files
from .config import UniMedVLConfig
from .data_utils import add_special_tokens, pil_img2rgb
from .shapes import all_shapes
from .transforms import ImageTransform

DEFAULT_CONFIG = {
    "model_path": "/path/to/unimedvl_checkpoint",
    "target_gpu_device": "0",
    "max_mem_per_gpu": "40GiB",
    "temperature": 1.0,
    "max_new_tokens": 512,
    "do_sample": True,
    "seed": 42,
    "enable_cpu_loading": True,
    "enable_auto_bf16_conversion": True,
    "use_model_checkpoint": False,  # False = ema.safetensors, True = model.safetensors
    "offload_folder": "/tmp/bagel_offload",
    # truncated sampling (not reference keys; off = the reference's full-softmax draw): Bagel.generate_text
    "top_k": 0,
    "top_p": 1.0,
    "min_p": 0.0,
    # logit penalties (not reference keys; off = the reference's logits): Bagel.generate_text
    "repetition_penalty": 1.0,
    "presence_penalty": 0.0,
    "frequency_penalty": 0.0,
    "logit_bias": None,
    "penalize_prompt": False,       # True: the prompt's own tokens (not the bos / eos wrapper) count as seen for repetition_penalty
    # no-repeat n-grams (not reference keys; 0 = off): the answer repeats no n-gram of that size (Bagel.chat); "no_repeat_ngram_prompt":
    # True also counts the n-grams of the prompt's own tokens (HF's generate does), False the generated tokens only
    "no_repeat_ngram_size": 0,
    "no_repeat_ngram_prompt": False,
    # banned sequences (not reference keys; None / 0 = off): HF's generate keywords of these names (Bagel.chat) - token lists the answer
    # must not hold, tokens it never / never first emits, and the number of tokens it holds before the end token may come; they also
    # run with "num_beams" > 1.  "bad_words": strings, each banned as the tokenizer encodes it bare and behind a space
    "bad_words_ids": None,
    "bad_words": None,
    "suppress_tokens": None,
    "begin_suppress_tokens": None,
    "min_new_tokens": 0,
    # speculative greedy decode (not reference keys; off = one token per step): Bagel.chat - needs "do_sample": False
    "draft_len": 0,                 # drafted tokens verified per step (prompt lookup over the question and the answer so far)
    "draft_ngram": (2, 4),
    # per-request sampling (not a reference key; None = the scalar keys above): a sampling.SamplingParams, or a dict of its fields - the
    # request's own sampler and seed (Bagel.chat(sampling=...)).  It REPLACES "do_sample" / "temperature" / "top_k" / "top_p" / "min_p"
    # and the three penalty keys, which are then not passed on; with "draft_len" > 0 it is sampled speculative decode
    "sampling": None,
    # guided choice (not a reference key; None = free text): a list of answers (strings or token-id lists) - the answer is one of them,
    # picked by the sampler the keys above set (Bagel.chat(choices=...)); "choices_after": "free" makes them answer PREFIXES.  `score`
    # ranks the same closed set exactly, at one forced row per candidate; this costs one row and returns the sampler's pick
    "choices": None,
    "choices_after": "stop",
    # beam search decode (not reference keys; "num_beams": 1 = off): HF's generate(num_beams=K, do_sample=False) with its
    # "length_penalty" and "early_stopping" (Bagel.chat) - needs "do_sample": False and none of the sampler, penalty, n-gram, draft and
    # choice keys above.  "num_return_sequences" > 1: the result also carries "answers", a list of (answer, score), best first
    "num_beams": 1,
    "length_penalty": 1.0,
    "early_stopping": False,
    "num_return_sequences": 1,
    # classifier-free guidance for text (not reference keys; "guidance_scale": 1.0 = off): HF's guidance_scale (Bagel.chat) - the answer
    # is decoded from the contrast of the question about the image with the same question WITHOUT the image ("negative_prompt": None;
    # visual contrastive decoding) or with a negative prompt (a string); "guidance_plausibility" (beta in [0, 1), 0 = off) first drops
    # the tokens the conditional distribution itself finds implausible.  Not with beams, drafts, "sampling", penalties, bans or choices
    "guidance_scale": 1.0,
    "negative_prompt": None,
    "guidance_plausibility": 0.0,
}

# codes/data/default.yaml vlm_sft.image_transform_args (read by eval/vlm/utils.py:486-502)
VLM_SFT_TRANSFORM = dict(max_image_size=980, min_image_size=378, image_stride=14, max_pixels=2_007_040)


def build_transform():
    return ImageTransform(**VLM_SFT_TRANSFORM)


def process_conversation(images, conversation):
    return [pil_img2rgb(image) for image in images], conversation


def load_tokenizer(model_path):
    """Qwen2 byte-level BPE from the checkpoint's vocab.json / merges.txt / tokenizer_config.json
    (Qwen2Tokenizer.from_pretrained(model_path), interactive_vqa_inferencer.py:236): the in-tree implementation,
    id-for-id equal to the reference's class (tests/test_tokenizer_cpu.py); no transformers import at run time."""
    from .tokenizer import Qwen2Tokenizer
    return Qwen2Tokenizer.from_pretrained(model_path)


class VQAInferencer:
    def __init__(self, config: Optional[Dict[str, Any]] = None):
        self.config = dict(DEFAULT_CONFIG)
        if config:
            self.config.update(config)
        self.model = None
        self.tokenizer = None
        self.new_token_ids = None
        self.image_transform = None
        self.loaded = False

    def set_seed(self, seed):
        import random
        import numpy as np
        random.seed(seed)
        np.random.seed(seed)
        torch.manual_seed(seed)
        if torch.cuda.is_available():
            torch.cuda.manual_seed_all(seed)

    def convert_checkpoint_to_bf16(self, input_path, output_path):
        """reference method of the same name (one-time fp32 -> bf16 checkpoint conversion); not needed by load_model() here"""
        from .checkpoint import convert_checkpoint_to_bf16
        return convert_checkpoint_to_bf16(input_path, output_path)

    def load_model(self, model=None, tokenizer=None, new_token_ids=None):
        """Builds the engine from ``config['model_path']``.  Pre-built objects may be injected
        (tests / benches without a checkpoint)."""
        if self.loaded:
            print("Model already loaded")
            return
        self.set_seed(self.config["seed"])
        if model is None:
            model_path = self.config.get("model_path")
            if not model_path:
                raise ValueError("model_path required")
            cfg = UniMedVLConfig.from_checkpoint_dir(model_path)
            device = f"cuda:{self.config['target_gpu_device']}"
            # optional extras over the reference's config keys: "checkpoint_weight_path" overlays a fine-tuned checkpoint on the
            # base one (eval/vlm/utils.py:71-98); "llm_weight_dtype": "fp8" / "fp4" streams e4m3 / MXFP4 LLM weights at decode
            cfg.llm_weight_dtype = self.config.get("llm_weight_dtype", "bf16")
            # "llm_fp4_keep_bf16": False (with "fp4") keeps only the MXFP4 images of the LLM linears: every row count runs on them
            cfg.llm_fp4_keep_bf16 = bool(self.config.get("llm_fp4_keep_bf16", True))
            get = checkpoint_getter(model_path, all_shapes(cfg), self.config.get("checkpoint_weight_path"),
                                    self.config["use_model_checkpoint"])
            # fast path (not a reference key; the counterpart of its one-time ema_bf16.safetensors conversion,
            # interactive_vqa_inferencer.py:93-161): "packed_cache" (default True) keeps the device-ready weight images in
            # <model_path>/ema_packed_*.safetensors after the first load and reads them back on every later one
            t_load = time.time()
            store = packstore.attach(get, self.config.get("checkpoint_weight_path") or model_path, device, cfg,
                                     checkpoint_source_files(model_path, self.config.get("checkpoint_weight_path"),
                                                             self.config["use_model_checkpoint"]),
                                     enabled=bool(self.config.get("packed_cache", True)), extra_tag="_und")
            model = Bagel(cfg, get, device=device, visual_gen=False, visual_und=True)
            torch.cuda.synchronize()
            self.load_stats = {"load_s": round(time.time() - t_load, 3), "packed_cache": store.status, "from_packed": store.hits,
                               "built": store.misses}
            t_save = store.save()
            if t_save is not None:
                self.load_stats.update(packed_cache=store.status, packed_cache_write_s=round(t_save, 3))
            print(f"weights: {self.load_stats}")
            tokenizer = load_tokenizer(model_path)
            tokenizer, new_token_ids, _ = add_special_tokens(tokenizer)
        self.model, self.tokenizer, self.new_token_ids = model, tokenizer, new_token_ids
        # serving extra (not a reference key): every request prefills / decodes in ONE reserved cache, so the image span of a
        # request whose patch grid was seen before replays from a HIP graph (Bagel.forward_cache_update_vit); 0 = a fresh cache
        # per request as in the reference (bagel.py:1341)
        if hasattr(self.model, "chat_cache_tokens"):
            self.model.chat_cache_tokens = int(self.config.get("serving_cache_tokens", 8192))
        self.image_transform = build_transform()
        self.loaded = True
        self.show_gpu_memory()

    def show_gpu_memory(self):
        if torch.cuda.is_available():
            for i in range(torch.cuda.device_count()):
                allocated = torch.cuda.memory_allocated(i) / 1024 ** 3
                total = torch.cuda.get_device_properties(i).total_memory / 1024 ** 3
                print(f"GPU {i}: {allocated:.1f}GB / {total:.1f}GB ({allocated / total * 100:.1f}%)")

    def cleanup_memory(self):
        if torch.cuda.is_available():
            torch.cuda.empty_cache()
        gc.collect()
        self.show_gpu_memory()

    def infer_single(self, image_path, prompt, temperature=None, max_new_tokens=None, do_sample=None, show_image=False, *,
                     repetition_penalty=None, presence_penalty=None, frequency_penalty=None, logit_bias=None, penalize_prompt=None,
                     draft_len=None, draft_ngram=None, predicted_ids=None, choices=None, top_k=None, top_p=None, min_p=None):
        if not self.loaded:
            raise RuntimeError("Model not loaded, please call load_model() first")
        temperature_arg, do_sample_arg, top_k_arg, top_p_arg, min_p_arg = temperature, do_sample, top_k, top_p, min_p
        temperature = temperature if temperature is not None else self.config["temperature"]
        max_new_tokens = max_new_tokens if max_new_tokens is not None else self.config["max_new_tokens"]
        do_sample = do_sample if do_sample is not None else self.config["do_sample"]
        top_k = top_k if top_k is not None else self.config.get("top_k", 0)
        top_p = top_p if top_p is not None else self.config.get("top_p", 1.0)
        min_p = min_p if min_p is not None else self.config.get("min_p", 0.0)
        given = dict(repetition_penalty=repetition_penalty, presence_penalty=presence_penalty, frequency_penalty=frequency_penalty,
                     logit_bias=logit_bias, penalize_prompt=penalize_prompt)
        penalties = {k: v if v is not None else self.config.get(k, DEFAULT_CONFIG[k]) for k, v in given.items()}
        if isinstance(image_path, Image.Image):
            input_image, image_path = image_path.convert("RGB"), None
        else:
            if not os.path.exists(image_path):
                raise FileNotFoundError(f"Image file not found: {image_path}")
            input_image = Image.open(image_path).convert("RGB")
        start = time.time()
        images, conversation = process_conversation([input_image], prompt)
        # "return_logprobs" (not a reference key; default off): the result also carries "token_ids" and "token_logprobs", the generated
        # tokens behind the answer and the log-probability of each (Bagel.generate_text).  Without it the result is the reference's.
        # "top_logprobs" (n, default 0 = off; implies "return_logprobs"): the result also carries "top_logprobs" - per token its n most
        # likely alternatives as (id, logprob) pairs - and "token_ranks", each token's own 1-based rank (Bagel.generate_text).
        n_top = int(self.config.get("top_logprobs", 0) or 0)
        want_lp = bool(self.config.get("return_logprobs", False)) or n_top > 0
        extra = {"return_logprobs": True} if want_lp else {}
        if n_top:
            extra["top_logprobs"] = n_top
        draft_len = draft_len if draft_len is not None else self.config.get("draft_len", 0)
        if draft_len:       # predicted_ids: a predicted answer (a string or token ids) to draft from instead of the lookup
            extra.update(draft_len=draft_len, draft_ngram=draft_ngram if draft_ngram is not None else self.config.get("draft_ngram", (2, 4)),
                         predicted_ids=predicted_ids)
        choices = choices if choices is not None else self.config.get("choices")
        if choices is not None:     # the answer is one of these (this call's list, else the config's); not with drafts (Bagel.generate_text)
            extra.update(choices=choices, choices_after=self.config.get("choices_after", "stop"))
        if self.config.get("no_repeat_ngram_size", 0):
            extra.update(no_repeat_ngram_size=self.config["no_repeat_ngram_size"])
        if self.config.get("no_repeat_ngram_prompt", False):      # (with "sampling" the size is the SamplingParams')
            extra.update(no_repeat_ngram_prompt=True)
        for key in ("bad_words_ids", "bad_words", "suppress_tokens", "begin_suppress_tokens", "min_new_tokens"):
            if self.config.get(key):
                extra[key] = self.config[key]
        if float(self.config.get("guidance_scale", 1.0)) != 1.0 or self.config.get("negative_prompt") is not None:
            extra.update({k: self.config.get(k, DEFAULT_CONFIG[k]) for k in ("guidance_scale", "negative_prompt", "guidance_plausibility")})
        sampler = dict(do_sample=do_sample, temperature=temperature, top_k=top_k, top_p=top_p, min_p=min_p, **penalties)
        sampling = self.config.get("sampling")
        if sampling is not None:    # the config's scalar sampler keys step aside; one given to this call explicitly is passed on (and refused)
            from .sampling import SamplingParams
            passed = dict(temperature=temperature_arg, do_sample=do_sample_arg, top_k=top_k_arg, top_p=top_p_arg, min_p=min_p_arg, **given)
            sampler = {k: v for k, v in passed.items() if v is not None and k not in ("logit_bias", "penalize_prompt")}
            sampler.update(sampling=sampling if isinstance(sampling, SamplingParams) else SamplingParams(**sampling),
                           logit_bias=penalties["logit_bias"], penalize_prompt=penalties["penalize_prompt"])
        answers = None
        if int(self.config.get("num_beams", 1) or 1) > 1:
            extra.update({k: self.config.get(k, DEFAULT_CONFIG[k]) for k in ("num_beams", "length_penalty", "early_stopping", "num_return_sequences")})
            if extra["num_return_sequences"] > 1:           # several answers: each comes with its score, not with per-token values
                extra.pop("return_logprobs", None)
                want_lp = False
        answer = self.model.chat(self.tokenizer, self.new_token_ids, self.image_transform, images=images,
                                 prompt=conversation, max_length=max_new_tokens, **sampler, **extra)
        if extra.get("num_return_sequences", 1) > 1:        # (answer, score) pairs, best first
            answers, answer = answer, answer[0][0]
        top = None
        if n_top:
            answer, token_ids, token_logprobs, top = answer
        elif want_lp:
            answer, token_ids, token_logprobs = answer
        result = {"answer": answer, "input_image": input_image, "time": time.time() - start, "image_path": image_path,
                  "prompt": prompt, "timestamp": datetime.now().strftime("%Y-%m-%d %H:%M:%S")}
        if answers is not None:
            result.update(answers=answers)
        if want_lp:
            result.update(token_ids=token_ids, token_logprobs=token_logprobs)
        if top is not None:
            result.update(top_logprobs=[list(zip(i, l)) for i, l in zip(top.ids, top.logprobs)], token_ranks=top.rank)
        return result

    def score(self, image, question, candidates, append_eos=True):
        """Closed-set answering (Bagel.score): one dict per candidate - token_ids, token_logprobs, logprob - for the answers
        `candidates` (strings or token-id lists, at most 64) to `question` about `image` (a PIL image or a path).  With the config key
        "top_logprobs" set (n, 0 included) every dict also carries token_ranks and, for n > 0, top_logprobs (Bagel.score)."""
        if not self.loaded:
            raise RuntimeError("Model not loaded, please call load_model() first")
        input_image = image.convert("RGB") if isinstance(image, Image.Image) else Image.open(image).convert("RGB")
        images, conversation = process_conversation([input_image], question)
        if self.config.get("top_logprobs") is not None:
            return self.model.score_top_logprobs(self.tokenizer, self.new_token_ids, self.image_transform, images, conversation, candidates,
                                                 append_eos=append_eos, top_logprobs=self.config["top_logprobs"])
        return self.model.score(self.tokenizer, self.new_token_ids, self.image_transform, images, conversation, candidates,
                                append_eos=append_eos)

    def score_prefill(self, image, question, candidates, append_eos=True):
        """`score` for long candidates (Bagel.score_prefill): the same dicts - token_ids, token_logprobs, logprob - from one prefill pass
        over all candidates' rows instead of one decode step per token.  No ranks or alternatives (the "top_logprobs" key is `score`'s)."""
        if not self.loaded:
            raise RuntimeError("Model not loaded, please call load_model() first")
        input_image = image.convert("RGB") if isinstance(image, Image.Image) else Image.open(image).convert("RGB")
        images, conversation = process_conversation([input_image], question)
        return self.model.score_prefill(self.tokenizer, self.new_token_ids, self.image_transform, images, conversation, candidates,
                                        append_eos=append_eos)
