"""ctypes binding of libunimedvl_hip.so (include/unimedvl_hip.h).

The product path has NO fallback: if the shared library is missing or a symbol
is absent this module raises, and every op raises on a non-zero return code.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("UMV_LIB_PATH") or os.path.join(HERE, "lib", "libunimedvl_hip.so")   # (override: A/B builds, tuning only)

EPI_BIAS, EPI_GELU_TANH, EPI_SILU, EPI_RESIDUAL, EPI_SWIGLU, EPI_OUT_F32 = 1, 2, 4, 8, 16, 32


class GemmArgs(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("ldx", C.c_int64), ("wp", C.c_void_p), ("bias", C.c_void_p),
        ("residual", C.c_void_p), ("ldr", C.c_int64), ("out", C.c_void_p), ("ldo", C.c_int64),
        ("row_idx", C.c_void_p), ("M", C.c_int), ("N", C.c_int), ("K", C.c_int), ("epilogue", C.c_int),
        ("norm_w", C.c_void_p), ("norm_eps", C.c_float), ("tile_rows", C.c_int), ("w_scale", C.c_void_p),
        ("k_splits", C.c_int), ("split_stride", C.c_int64), ("argmax_partial", C.c_void_p), ("x_rows", C.c_int64),
        ("sample_temperature", C.c_float), ("sample_seed", C.c_uint64), ("sample_step", C.c_void_p),
        ("lse_partial", C.c_void_p),
    ]


class QkvPostArgs(C.Structure):
    _fields_ = [
        ("qkv", C.c_void_p), ("q_out", C.c_void_p), ("k_slab", C.c_void_p), ("vt_slab", C.c_void_p),
        ("k_seg_stride", C.c_int64), ("k_head_stride", C.c_int64), ("v_seg_stride", C.c_int64),
        ("v_head_stride", C.c_int64), ("v_d_stride", C.c_int64),
        ("tok_seg", C.c_void_p), ("tok_slot", C.c_void_p), ("tok_pos", C.c_void_p), ("expert", C.c_void_p),
        ("q_norm_w", C.c_void_p), ("k_norm_w", C.c_void_p), ("q_norm_w_gen", C.c_void_p), ("k_norm_w_gen", C.c_void_p),
        ("cos_tab", C.c_void_p), ("sin_tab", C.c_void_p),
        ("T", C.c_int), ("nq", C.c_int), ("nkv", C.c_int), ("hd", C.c_int), ("eps", C.c_float),
        ("fp32_chain", C.c_int),
        ("qkv_partials", C.c_void_p), ("n_splits", C.c_int), ("split_stride", C.c_int64), ("qkv_bias", C.c_void_p),
        ("page_table", C.c_void_p), ("page_table_stride", C.c_int),
    ]


class AttnArgs(C.Structure):
    _fields_ = [
        ("q", C.c_void_p), ("out", C.c_void_p), ("cu_q", C.c_void_p), ("kv_len", C.c_void_p),
        ("k_slab", C.c_void_p), ("vt_slab", C.c_void_p),
        ("k_seg_stride", C.c_int64), ("k_head_stride", C.c_int64), ("v_seg_stride", C.c_int64),
        ("v_head_stride", C.c_int64), ("v_d_stride", C.c_int64),
        ("nseg", C.c_int), ("nq", C.c_int), ("nkv", C.c_int), ("hd", C.c_int), ("causal", C.c_int),
        ("max_q", C.c_int), ("max_kv", C.c_int), ("nsplit", C.c_int), ("workspace", C.c_void_p),
        ("q_row_stride", C.c_int64), ("k_key_stride", C.c_int64),
        ("variant", C.c_int), ("stats", C.c_void_p),
        ("page_table", C.c_void_p), ("page_table_stride", C.c_int), ("wave_split", C.c_int),
    ]


# umv_attn_args.variant bits (tests / A-B only): FORCE makes the others replace the library's shape -> kernel policy for one call
ATTN_FORCE, ATTN_STREAM, ATTN_TQ1, ATTN_TQ2, ATTN_EXACT, ATTN_WHOLE_TOKENS = 1, 2, 4, 8, 16, 32
ATTN_PAIR = 64      # once: both q-tiles of a wave in one softmax call.  The library ignores the bit now; the name stays so that callers written against it still load


class Gemm8Args(C.Structure):
    _fields_ = [
        ("xq", C.c_void_p), ("ldq", C.c_int64), ("x_scale", C.c_void_p), ("wp", C.c_void_p), ("w_scale", C.c_void_p),
        ("bias", C.c_void_p), ("residual", C.c_void_p), ("ldr", C.c_int64), ("out", C.c_void_p), ("ldo", C.c_int64),
        ("row_idx", C.c_void_p), ("M", C.c_int), ("N", C.c_int), ("K", C.c_int), ("epilogue", C.c_int),
    ]


class LogitPenaltyArgs(C.Structure):
    _fields_ = [
        ("logits", C.c_void_p), ("ld", C.c_int64), ("ids", C.c_void_p), ("count", C.c_void_p), ("list", C.c_void_p),
        ("list_len", C.c_void_p), ("bias", C.c_void_p), ("M", C.c_int), ("V", C.c_int), ("cap", C.c_int), ("n_static", C.c_int),
        ("repetition_penalty", C.c_float), ("presence_penalty", C.c_float), ("frequency_penalty", C.c_float),
        ("temperature", C.c_float), ("argmax_partial", C.c_void_p), ("lse_partial", C.c_void_p), ("n_tiles", C.c_int),
        ("seed", C.c_uint64), ("step", C.c_void_p), ("rows", C.c_void_p),
    ]


class TokenAutomatonArgs(C.Structure):
    """umv_token_automaton: a token automaton in CSR form, device pointers (constraints.TokenAutomaton.to_device)"""
    _fields_ = [
        ("row_ptr", C.c_void_p), ("edge_token", C.c_void_p), ("edge_next", C.c_void_p), ("n_states", C.c_int), ("n_edges", C.c_int),
    ]


class LogitConstrainArgs(C.Structure):
    _fields_ = [
        ("logits", C.c_void_p), ("ld", C.c_int64), ("M", C.c_int), ("V", C.c_int), ("automaton", TokenAutomatonArgs),
        ("state", C.c_void_p), ("temperature", C.c_float), ("argmax_partial", C.c_void_p), ("lse_partial", C.c_void_p),
        ("n_tiles", C.c_int), ("seed", C.c_uint64), ("step", C.c_void_p), ("rows", C.c_void_p),
    ]


class NgramBanArgs(C.Structure):
    """umv_ngram_ban_args: no_repeat_ngram_size on the stored logits of a step (umv_logit_ngram_ban_bf16)"""
    _fields_ = [
        ("logits", C.c_void_p), ("ld", C.c_int64), ("ids", C.c_void_p), ("hist", C.c_void_p), ("hist_ld", C.c_int64),
        ("hist_len", C.c_void_p), ("row_n", C.c_void_p), ("M", C.c_int), ("V", C.c_int), ("n", C.c_int), ("temperature", C.c_float),
        ("argmax_partial", C.c_void_p), ("lse_partial", C.c_void_p), ("n_tiles", C.c_int), ("seed", C.c_uint64), ("step", C.c_void_p),
        ("rows", C.c_void_p),
    ]


class RowSampling(C.Structure):
    """umv_row_sampling: one row of the per-row sampling table (device memory; sampling.ROW_DTYPE is the same layout for numpy)"""
    _fields_ = [
        ("seed", C.c_uint64), ("draw", C.c_int64), ("stream", C.c_uint32), ("temperature", C.c_float), ("top_k", C.c_int32),
        ("top_p", C.c_float), ("min_p", C.c_float), ("repetition_penalty", C.c_float), ("presence_penalty", C.c_float),
        ("frequency_penalty", C.c_float),
    ]


class SpecStepArgs(C.Structure):
    """umv_spec_step_args: the step end of a speculative decode step (umv_decode_step_end_speculative)"""
    _fields_ = [
        ("tok_slot", C.c_void_p), ("tok_pos", C.c_void_p), ("kv_len", C.c_void_p), ("argmax_partial", C.c_void_p),
        ("n_tiles", C.c_int), ("V", C.c_int), ("ids", C.c_void_p), ("out_ids", C.c_void_p), ("out_ld", C.c_int64),
        ("n_out", C.c_void_p), ("limit", C.c_void_p), ("n_draft", C.c_void_p), ("hist", C.c_void_p), ("hist_ld", C.c_int64),
        ("hist_len", C.c_void_p), ("predicted", C.c_void_p), ("pred_ld", C.c_int64), ("pred_len", C.c_void_p), ("stats", C.c_void_p),
        ("B", C.c_int), ("k", C.c_int), ("ngram_min", C.c_int), ("ngram_max", C.c_int), ("draft_only", C.c_int),
    ]


class SpecRowsStepArgs(C.Structure):
    """umv_spec_rows_step_args: the commit launch of a sampled speculative step (umv_decode_step_end_speculative_rows)"""
    _fields_ = [
        ("step", SpecStepArgs), ("picks", C.c_void_p), ("rows", C.c_void_p), ("row_logprob", C.c_void_p), ("out_logprobs", C.c_void_p),
    ]


class BeamStepArgs(C.Structure):
    """umv_beam_step_args: the step end of a beam search step (umv_beam_step_end)"""
    _fields_ = [
        ("tok_slot", C.c_void_p), ("tok_pos", C.c_void_p), ("kv_len", C.c_void_p), ("ids", C.c_void_p), ("step_idx", C.c_void_p),
        ("cand_ids", C.c_void_p), ("cand_lp", C.c_void_p), ("scores", C.c_void_p), ("beam_tok", C.c_void_p), ("beam_parent", C.c_void_p),
        ("beam_lp", C.c_void_p), ("fin_f", C.c_void_p), ("fin_i", C.c_void_p), ("hdr", C.c_void_p), ("len_norm", C.c_void_p),
        ("table", C.c_void_p), ("own", C.c_void_p), ("j0", C.c_void_p), ("copies", C.c_void_p),
        ("table_stride", C.c_int32), ("n_own", C.c_int32), ("B", C.c_int32), ("K", C.c_int32), ("max_len", C.c_int32),
        ("end_token_id", C.c_int32), ("early_stopping", C.c_int32),
    ]


class SequenceBanArgs(C.Structure):
    """umv_sequence_ban_args: banned sequences on the stored logits of a step (umv_logit_sequence_ban_bf16)"""
    _fields_ = [
        ("logits", C.c_void_p), ("ld", C.c_int64), ("ids", C.c_void_p), ("seq_ptr", C.c_void_p), ("seq_tok", C.c_void_p),
        ("seq_until", C.c_void_p), ("row_min", C.c_void_p), ("tail", C.c_void_p), ("count", C.c_void_p), ("beam_tok", C.c_void_p),
        ("beam_parent", C.c_void_p), ("step_idx", C.c_void_p), ("start_ids", C.c_void_p),
        ("M", C.c_int), ("V", C.c_int), ("S", C.c_int), ("n_tok", C.c_int), ("max_m", C.c_int), ("K", C.c_int), ("max_len", C.c_int),
        ("temperature", C.c_float), ("argmax_partial", C.c_void_p), ("lse_partial", C.c_void_p), ("n_tiles", C.c_int),
        ("seed", C.c_uint64), ("step", C.c_void_p), ("rows", C.c_void_p),
    ]


class LogitGuidanceArgs(C.Structure):
    """umv_logit_guidance_args: classifier-free guidance for text on the stored logits of a step (umv_logit_guidance_bf16)"""
    _fields_ = [
        ("logits", C.c_void_p), ("ld", C.c_int64), ("M", C.c_int), ("V", C.c_int), ("pair", C.c_void_p), ("scale", C.c_void_p),
        ("log_beta", C.c_void_p), ("lse", C.c_void_p), ("row_max", C.c_void_p), ("stats", C.c_void_p), ("temperature", C.c_float),
        ("argmax_partial", C.c_void_p), ("lse_partial", C.c_void_p), ("n_tiles", C.c_int), ("seed", C.c_uint64), ("step", C.c_void_p),
    ]


# beam search decode: the most beams a request can have, and the full-page table entries one request's step end can carry (K * n_own)
BEAM_K_MAX, BEAM_TABLE_ENTRIES = 10, 1024
# umv_logit_penalty_args.count words: bits 0..29 the count, then "in the context set" and "in the row's visit list"
PENALTY_COUNT_MASK, PENALTY_CONTEXT, PENALTY_LISTED = 0x3FFFFFFF, 0x40000000, 0x80000000
# umv_decode_top_logprobs: the most alternatives a row can ask for, and the step end whose merge order the statistics take
TOP_LOGPROBS_MAX, TOP_AFTER_LOGPROB, TOP_AFTER_TRUNCATED = 20, 0, 1
# token automata: the state words of a released row and of a row that was fed a token outside its state's edges; the columns one
# workgroup of umv_logit_constrain_bf16 masks (UMV_CONSTRAIN_CHUNK)
CONSTRAINT_FREE, CONSTRAINT_LEFT, CONSTRAIN_CHUNK = -1, -2, 4096
# no-repeat n-grams: the largest size a row can ask for, and the length word of a row whose history ran full (UMV_NGRAM_FULL)
NGRAM_MAX, NGRAM_FULL = 16, -2
# banned sequences: the longest entry, the most entries, and the `until` word of an entry that holds while count <= row_min[b]
SEQ_MAX, SEQ_ENTRIES_MAX, SEQ_ROW = 16, 4096, -1


_SIGS = {
    "umv_packed_weight_fp8_mfma_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "umv_repack_weight_fp8_mfma": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "umv_quantize_act_fp8": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                       C.c_int, C.c_int, C.c_void_p]),
    "umv_gemm_fp8a8w": (C.c_int, [C.POINTER(Gemm8Args), C.c_void_p]),
    "umv_gemm_tile_config": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "umv_attn_prefill_tq": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "umv_version": (C.c_int, []),
    "umv_last_error": (C.c_char_p, []),
    "umv_packed_weight_elems": (C.c_size_t, [C.c_int, C.c_int]),
    "umv_pack_weight_bf16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "umv_repacked_weight_elems": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "umv_repack_weight_rows_bf16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "umv_pack_weight_swiglu_bf16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "umv_gemm_bf16": (C.c_int, [C.POINTER(GemmArgs), C.c_void_p]),
    "umv_packed_weight_fp8_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "umv_quantize_pack_weight_fp8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_int, C.c_int, C.c_void_p]),
    "umv_gemm_fp8w": (C.c_int, [C.POINTER(GemmArgs), C.c_void_p]),
    "umv_gemm_bf16_rows": (C.c_int, [C.POINTER(GemmArgs), C.c_void_p, C.c_void_p]),
    "umv_gemm_fp8w_rows": (C.c_int, [C.POINTER(GemmArgs), C.c_void_p, C.c_void_p]),
    "umv_gemm_z13w_rows": (C.c_int, [C.POINTER(GemmArgs), C.c_void_p, C.c_void_p, C.c_void_p]),
    "umv_packed_weight_mxfp4_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "umv_quantize_pack_weight_mxfp4": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                                 C.c_void_p]),
    "umv_gemm_mxfp4w": (C.c_int, [C.POINTER(GemmArgs), C.c_void_p]),
    "umv_packed_weight_z13_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "umv_pack_weight_z13": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "umv_gemm_z13w": (C.c_int, [C.POINTER(GemmArgs), C.c_void_p, C.c_void_p]),
    "umv_gemm_mxfp4t": (C.c_int, [C.POINTER(GemmArgs), C.c_void_p]),
    "umv_residual_rmsnorm_bf16": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                            C.c_int, C.c_float, C.c_void_p]),
    "umv_rmsnorm_bf16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                   C.c_float, C.c_void_p]),
    "umv_layernorm_bf16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float,
                                     C.c_void_p]),
    "umv_embed_gather_bf16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "umv_add_rows_bf16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                    C.c_int, C.c_void_p]),
    "umv_argmax_bf16": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "umv_sample_bf16": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_uint64, C.c_void_p,
                                  C.c_void_p]),
    "umv_cast_pad_f32_bf16": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int,
                                        C.c_void_p]),
    "umv_patchify_f32_bf16": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]),
    "umv_qkv_post": (C.c_int, [C.POINTER(QkvPostArgs), C.c_void_p]),
    "umv_attn_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "umv_attn_varlen": (C.c_int, [C.POINTER(AttnArgs), C.c_void_p]),
    "umv_decode_advance": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "umv_decode_step_end": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                      C.c_int, C.c_void_p]),
    "umv_decode_step_end_argmax": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "umv_decode_step_end_logprob": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_float, C.c_void_p, C.c_void_p,
                                              C.c_int, C.c_int, C.c_void_p]),
    "umv_token_logprob_bf16": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p]),
    "umv_lm_head_stats_bf16": (C.c_int, [C.POINTER(GemmArgs), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "umv_token_logprob_from_stats": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "umv_sample_truncated_bf16": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_uint64, C.c_void_p,
                                            C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "umv_decode_step_end_truncated": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_float, C.c_void_p, C.c_void_p,
                                                C.c_int, C.c_int, C.c_uint64, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p,
                                                C.c_void_p]),
    "umv_decode_step_end_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "umv_decode_top_logprobs": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_int, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "umv_top_logprobs_bf16": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p]),
    "umv_logit_penalty_bf16": (C.c_int, [C.POINTER(LogitPenaltyArgs), C.c_void_p]),
    "umv_logit_constrain_bf16": (C.c_int, [C.POINTER(LogitConstrainArgs), C.c_void_p]),
    "umv_constraint_advance": (C.c_int, [C.POINTER(TokenAutomatonArgs), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "umv_logit_ngram_ban_bf16": (C.c_int, [C.POINTER(NgramBanArgs), C.c_void_p]),
    "umv_decode_step_end_speculative": (C.c_int, [C.POINTER(SpecStepArgs), C.c_void_p]),
    "umv_decode_pick_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "umv_decode_step_end_speculative_rows": (C.c_int, [C.POINTER(SpecRowsStepArgs), C.c_void_p]),
    "umv_beam_candidates": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p]),
    "umv_beam_step_end": (C.c_int, [C.POINTER(BeamStepArgs), C.c_void_p]),
    "umv_logit_sequence_ban_bf16": (C.c_int, [C.POINTER(SequenceBanArgs), C.c_void_p]),
    "umv_logit_guidance_bf16": (C.c_int, [C.POINTER(LogitGuidanceArgs), C.c_void_p]),
    "umv_guidance_feed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "umv_beam_kv_copy": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "umv_timestep_embed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "umv_cfg_renorm_euler": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                       C.c_int, C.c_float, C.c_float, C.c_float, C.c_int, C.c_float, C.c_int, C.c_void_p]),
    "umv_conv2d_nhwc_bf16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                       C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "umv_groupnorm_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "umv_groupnorm_nhwc_bf16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                          C.c_int, C.c_float, C.c_int, C.c_void_p]),
    "umv_nchw_f32_to_nhwc_bf16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                            C.c_void_p]),
    "umv_unpatchify_latent": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                        C.c_float, C.c_void_p]),
    "umv_pixels_to_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]),
    "umv_softmax_rows_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p]),
    "umv_rowscale_f32_bf16": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p]),
    "umv_latent_sample_patchify": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                             C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p]),
}

_lib = None


class UmvError(RuntimeError):
    pass


def load():
    """Load the library once; raises if it (or any declared symbol) is missing."""
    global _lib
    if _lib is not None:
        return _lib
    # torch bundles its own HIP runtime (torch/lib/libamdhip64.so); importing torch first makes
    # the dynamic loader bind our library to THAT runtime instance, so device pointers and
    # streams are shared.  Loading ours first would pull a second runtime from /opt/rocm.
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise UmvError(
            f"{LIB_PATH} not found: build it with `python -m unimedvl_amd.build` "
            "(there is no CPU or PyTorch fallback for the product path)")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def declared_symbols():
    return list(_SIGS.keys())


def check(rc, what):
    if rc != 0:
        msg = load().umv_last_error().decode()
        raise UmvError(f"{what} failed (rc={rc}): {msg}")
