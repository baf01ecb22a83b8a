// Sanitizer driver for the C-ABI shim of libunimedvl_hip (SURVEY.md section 5 "race detection / sanitizers"; VERDICT r05 "missing" #4).
// Linked against a HOST-sanitized build of the library (tools/sanitize_abi.sh: -fsanitize=address,undefined resp. -fsanitize=thread, the
// device code is not instrumented).  It needs no GPU: it exercises everything the shim does BEFORE a launch -
//   * every host-only query over a sweep of shapes (sizes, tile / kernel policies: the lazily initialised, read-once policies),
//   * every entry point with NULL structs, NULL pointers and out-of-range dimensions (the UMV_CHECK paths, the thread-local error text),
//   * M = 0 / T = 0 early returns,
// first on one thread, then on 8 threads at once (ThreadSanitizer: the error buffer is thread-local, the policies are immutable after a
// thread-safe first use).  Exit code 0 = no entry point crashed, returned success for invalid input, or left the error text empty.
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <thread>
#include <vector>
#include <atomic>
#include "../include/unimedvl_hip.h"

static std::atomic<int> failures{0};
#define EXPECT_ERR(call)                                                                                  \
    do {                                                                                                  \
        const int rc__ = (call);                                                                          \
        const char* e__ = umv_last_error();                                                               \
        if (rc__ >= 0 || !e__ || !e__[0]) { ++failures; std::fprintf(stderr, "FAIL %s -> %d '%s'\n", #call, rc__, e__ ? e__ : "(null)"); } \
    } while (0)
#define EXPECT_OK(call)                                                                                   \
    do {                                                                                                  \
        const int rc__ = (call);                                                                          \
        if (rc__ != 0) { ++failures; std::fprintf(stderr, "FAIL %s -> %d '%s'\n", #call, rc__, umv_last_error()); } \
    } while (0)

static void queries() {
    size_t acc = 0;
    for (int n : {1, 16, 17, 1152, 3584, 4608, 37888, 152064})
        for (int k : {8, 32, 608, 1152, 3584, 18944}) {
            acc += umv_packed_weight_elems(n, k) + umv_packed_weight_fp8_bytes(n, k) + umv_packed_weight_fp8_mfma_bytes(n, k) + umv_packed_weight_mxfp4_bytes(n, k) +
                   umv_packed_weight_z13_bytes(n, k);
            for (int th : {1, 9, 14, 16}) acc += umv_repacked_weight_elems(n, k, th);
            for (int m : {1, 8, 64, 65, 272, 1026, 2064, 8208, 16500}) acc += (size_t)umv_gemm_tile_config(m, n, k);
        }
    for (int nseg : {1, 8, 32})
        for (int maxq : {1, 34, 258, 1026, 4096}) {
            acc += (size_t)umv_attn_prefill_tq(nseg, 28, 4, 128, maxq) + (size_t)umv_attn_prefill_tq(nseg, 16, 16, 72, maxq) + (size_t)umv_attn_prefill_tq(nseg, 2, 1, 64, maxq);
            for (int ns : {1, 4, 24}) acc += umv_attn_workspace_bytes(nseg, 28, 128, maxq, ns);
        }
    acc += umv_groupnorm_workspace_bytes(4, 256 * 256) + (size_t)umv_version();
    if (acc == 0) ++failures;
}

static void bad_arguments() {
    uint16_t dummy16[64] = {0};
    float dummyf[64] = {0};
    int32_t dummyi[64] = {0};
    int64_t dummyl[64] = {0};
    uint8_t dummy8[64] = {0};
    // GEMMs
    EXPECT_ERR(umv_gemm_bf16(nullptr, nullptr));
    umv_gemm_args g;
    std::memset(&g, 0, sizeof g);
    EXPECT_ERR(umv_gemm_bf16(&g, nullptr));                     // null x / wp / out
    g.x = dummy16; g.wp = dummy16; g.out = dummy16; g.M = 8; g.N = 16; g.K = 12;       // K % 8 != 0
    EXPECT_ERR(umv_gemm_bf16(&g, nullptr));
    g.K = 32; g.k_splits = 3; g.epilogue = UMV_EPI_SWIGLU;     // split-K with SwiGLU
    EXPECT_ERR(umv_gemm_bf16(&g, nullptr));
    EXPECT_ERR(umv_gemm_fp8w(nullptr, nullptr));
    std::memset(&g, 0, sizeof g);
    EXPECT_ERR(umv_gemm_fp8w(&g, nullptr));
    EXPECT_ERR(umv_gemm_mxfp4w(nullptr, nullptr));
    EXPECT_ERR(umv_gemm_mxfp4w(&g, nullptr));                  // null x / wp / out
    g.x = dummy16; g.wp = dummy16; g.out = dummy16; g.M = 8; g.N = 16; g.K = 48;       // K % 32 != 0
    EXPECT_ERR(umv_gemm_mxfp4w(&g, nullptr));
    g.K = 64; g.M = 65;                                         // the decode layout only
    EXPECT_ERR(umv_gemm_mxfp4w(&g, nullptr));
    g.M = 8; g.w_scale = dummyf;                                // the scales are part of the image
    EXPECT_ERR(umv_gemm_mxfp4w(&g, nullptr));
    g.w_scale = nullptr; g.argmax_partial = (uint64_t*)dummyl;  // lm_head stays e4m3
    EXPECT_ERR(umv_gemm_mxfp4w(&g, nullptr));
    EXPECT_ERR(umv_gemm_mxfp4t(nullptr, nullptr));
    std::memset(&g, 0, sizeof g);
    EXPECT_ERR(umv_gemm_mxfp4t(&g, nullptr));                  // null x / wp / out
    g.x = dummy16; g.wp = dummy16; g.out = dummy16; g.M = 65; g.N = 16; g.K = 48;      // K % 32 != 0
    EXPECT_ERR(umv_gemm_mxfp4t(&g, nullptr));
    g.K = 64; g.M = 64;                                         // the tiled kernel starts at 65 rows
    EXPECT_ERR(umv_gemm_mxfp4t(&g, nullptr));
    g.M = 65; g.w_scale = dummyf;                               // the scales are part of the image
    EXPECT_ERR(umv_gemm_mxfp4t(&g, nullptr));
    g.w_scale = nullptr; g.norm_w = dummy16;                    // no fused norm
    EXPECT_ERR(umv_gemm_mxfp4t(&g, nullptr));
    g.norm_w = nullptr; g.argmax_partial = (uint64_t*)dummyl;   // lm_head stays e4m3
    EXPECT_ERR(umv_gemm_mxfp4t(&g, nullptr));
    EXPECT_ERR(umv_gemm_z13w(nullptr, nullptr, nullptr));
    std::memset(&g, 0, sizeof g);
    EXPECT_ERR(umv_gemm_z13w(&g, dummy8, nullptr));             // null x / wp / out
    g.x = dummy16; g.wp = dummy16; g.out = dummy16; g.M = 8; g.N = 16; g.K = 64;
    EXPECT_ERR(umv_gemm_z13w(&g, nullptr, nullptr));            // no 13-bit image
    g.K = 96;                                                   // K % 64 != 0
    EXPECT_ERR(umv_gemm_z13w(&g, dummy8, nullptr));
    g.K = 64; g.M = 65;                                         // the decode layout only
    EXPECT_ERR(umv_gemm_z13w(&g, dummy8, nullptr));
    g.M = 8; g.norm_w = dummy16;                                // no fused norm
    EXPECT_ERR(umv_gemm_z13w(&g, dummy8, nullptr));
    g.norm_w = nullptr; g.tile_rows = 14;                       // 16-row images only
    EXPECT_ERR(umv_gemm_z13w(&g, dummy8, nullptr));
    g.tile_rows = 0; g.lse_partial = dummyf;                    // the softmax statistics ride on the argmax keys
    EXPECT_ERR(umv_gemm_z13w(&g, dummy8, nullptr));
    EXPECT_ERR(umv_gemm_bf16(&g, nullptr));
    EXPECT_ERR(umv_gemm_fp8w(&g, nullptr));
    std::memset(&g, 0, sizeof g);
    EXPECT_ERR(umv_gemm_fp8a8w(nullptr, nullptr));
    umv_gemm8_args g8;
    std::memset(&g8, 0, sizeof g8);
    EXPECT_ERR(umv_gemm_fp8a8w(&g8, nullptr));
    // packing / quantising
    EXPECT_ERR(umv_pack_weight_bf16(nullptr, nullptr, 16, 32, nullptr));
    EXPECT_ERR(umv_repack_weight_rows_bf16(nullptr, nullptr, 16, 32, 14, nullptr));
    EXPECT_ERR(umv_pack_weight_swiglu_bf16(nullptr, nullptr, nullptr, 16, 32, nullptr));
    EXPECT_ERR(umv_quantize_pack_weight_fp8(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 16, 512, nullptr));
    EXPECT_ERR(umv_repack_weight_fp8_mfma(nullptr, nullptr, 16, 128, nullptr));
    EXPECT_ERR(umv_quantize_pack_weight_mxfp4(nullptr, nullptr, nullptr, nullptr, nullptr, 16, 512, nullptr));
    EXPECT_ERR(umv_quantize_pack_weight_mxfp4(dummy16, nullptr, dummy8, nullptr, nullptr, 16, 48, nullptr));     // K % 32 != 0
    EXPECT_ERR(umv_quantize_pack_weight_mxfp4(dummy16, dummy16, dummy8, nullptr, nullptr, 17, 64, nullptr));     // SwiGLU I % 16
    EXPECT_ERR(umv_pack_weight_z13(nullptr, nullptr, 16, 64, nullptr));
    EXPECT_ERR(umv_pack_weight_z13(dummy16, dummy8, 16, 96, nullptr));                                           // K % 64 != 0
    EXPECT_ERR(umv_quantize_act_fp8(nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, 0, 8, 128, nullptr));
    // attention / qkv_post
    EXPECT_ERR(umv_attn_varlen(nullptr, nullptr));
    umv_attn_args a;
    std::memset(&a, 0, sizeof a);
    EXPECT_ERR(umv_attn_varlen(&a, nullptr));
    a.q = dummy16; a.out = dummy16; a.cu_q = dummyi; a.kv_len = dummyi; a.k_slab = dummy16; a.vt_slab = dummy16;
    a.nseg = 1; a.nq = 28; a.nkv = 5; a.hd = 128; a.max_q = 1; a.max_kv = 32; a.nsplit = 1;        // nq % nkv != 0
    EXPECT_ERR(umv_attn_varlen(&a, nullptr));
    a.nkv = 4; a.nsplit = 4;                                     // split without a workspace
    EXPECT_ERR(umv_attn_varlen(&a, nullptr));
    a.nsplit = 1; a.v_d_stride = 36;                             // capacity not a multiple of 8
    EXPECT_ERR(umv_attn_varlen(&a, nullptr));
    a.v_d_stride = 64; a.k_key_stride = 3584; a.causal = 1;      // packed K is the non-causal form
    EXPECT_ERR(umv_attn_varlen(&a, nullptr));
    a.k_key_stride = 0; a.causal = 0; a.page_table = dummyi; a.page_table_stride = 0;               // page table without a stride
    EXPECT_ERR(umv_attn_varlen(&a, nullptr));
    a.page_table = nullptr; a.nseg = 0;
    EXPECT_OK(umv_attn_varlen(&a, nullptr));                     // nothing to do
    EXPECT_ERR(umv_qkv_post(nullptr, nullptr));
    umv_qkv_post_args p;
    std::memset(&p, 0, sizeof p);
    EXPECT_ERR(umv_qkv_post(&p, nullptr));
    p.qkv = dummy16; p.q_out = dummy16; p.k_slab = dummy16; p.vt_slab = dummy16; p.tok_seg = dummyi; p.tok_slot = dummyi;
    p.q_norm_w = dummy16; p.T = 4; p.nq = 28; p.nkv = 4; p.hd = 128;                                   // norm without rope tables
    EXPECT_ERR(umv_qkv_post(&p, nullptr));
    // row kernels
    EXPECT_ERR(umv_rmsnorm_bf16(nullptr, nullptr, nullptr, nullptr, nullptr, 8, 3584, 1e-6f, nullptr));
    EXPECT_ERR(umv_residual_rmsnorm_bf16(nullptr, 4, 0, 0, nullptr, nullptr, nullptr, 8, 3584, 1e-6f, nullptr));
    EXPECT_ERR(umv_layernorm_bf16(nullptr, nullptr, nullptr, nullptr, 8, 1152, 1e-6f, nullptr));
    EXPECT_ERR(umv_layernorm_bf16(dummy16, dummy16, dummy16, dummy16, 8, 1153, 1e-6f, nullptr));    // H % 8 != 0
    EXPECT_ERR(umv_embed_gather_bf16(nullptr, nullptr, nullptr, nullptr, 8, 3584, nullptr));
    EXPECT_ERR(umv_add_rows_bf16(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 8, 3584, nullptr));
    EXPECT_ERR(umv_argmax_bf16(nullptr, 0, nullptr, 8, 152064, nullptr));
    EXPECT_ERR(umv_sample_bf16(nullptr, 0, nullptr, 8, 152064, 1.0f, 1, nullptr, nullptr));
    EXPECT_ERR(umv_sample_bf16(dummy16, 64, dummyl, 1, 64, 0.0f, 1, nullptr, nullptr));           // temperature 0
    EXPECT_OK(umv_sample_bf16(dummy16, 64, dummyl, 0, 64, 1.0f, 1, nullptr, nullptr));             // no rows
    EXPECT_ERR(umv_cast_pad_f32_bf16(nullptr, 0, nullptr, 0, 8, 588, 608, nullptr));
    EXPECT_ERR(umv_cast_pad_f32_bf16(dummyf, 588, dummy16, 608, 8, 588, 580, nullptr));            // Kp < K
    EXPECT_ERR(umv_patchify_f32_bf16(nullptr, 3, 448, 448, 14, nullptr, 608, 608, nullptr));
    EXPECT_ERR(umv_patchify_f32_bf16(dummyf, 3, 450, 448, 14, dummy16, 608, 608, nullptr));        // not whole patches
    EXPECT_ERR(umv_decode_advance(nullptr, nullptr, nullptr, 8, nullptr));
    EXPECT_ERR(umv_decode_step_end(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 8, 16, nullptr));
    EXPECT_ERR(umv_decode_step_end_argmax(nullptr, nullptr, nullptr, nullptr, 9504, nullptr, nullptr, nullptr, nullptr, 8, 16, nullptr));
    EXPECT_ERR(umv_decode_step_end_logprob(nullptr, nullptr, nullptr, nullptr, nullptr, 9504, nullptr, nullptr, nullptr, nullptr, nullptr, 152064,
                                           152064, 0.f, nullptr, nullptr, 8, 16, nullptr));
    EXPECT_ERR(umv_decode_step_end_logprob(dummyi, dummyi, dummyi, (const uint64_t*)dummyl, dummyf, 4, dummyl, dummyl, dummyl, dummyl, dummy16, 64,
                                           100, 0.f, nullptr, dummyf, 1, 16, nullptr));           // 100 columns are not 4 tiles
    EXPECT_ERR(umv_decode_step_end_logprob(dummyi, dummyi, dummyi, (const uint64_t*)dummyl, dummyf, 4, dummyl, dummyl, dummyl, dummyl, dummy16, 64,
                                           64, -1.f, nullptr, dummyf, 1, 16, nullptr));           // negative temperature
    EXPECT_ERR(umv_token_logprob_bf16(nullptr, 0, nullptr, nullptr, 8, 152064, 0.f, nullptr));
    EXPECT_ERR(umv_token_logprob_bf16(dummy16, 32, dummyl, dummyf, 1, 64, 0.f, nullptr));         // row stride below V
    EXPECT_ERR(umv_token_logprob_bf16(dummy16, 64, dummyl, dummyf, 1, 64, -1.f, nullptr));        // negative temperature
    EXPECT_OK(umv_token_logprob_bf16(dummy16, 64, dummyl, dummyf, 0, 64, 0.f, nullptr));          // no rows
    {   // the prefill-time scorer: the lm_head call that stores statistics instead of logits, and its finish
        umv_gemm_args gs;
        std::memset(&gs, 0, sizeof gs);
        gs.x = dummy16; gs.wp = dummy16; gs.ldx = 64; gs.M = 1; gs.N = 64; gs.K = 64;
        EXPECT_ERR(umv_lm_head_stats_bf16(nullptr, dummyl, dummyf, dummyf, nullptr));
        EXPECT_ERR(umv_lm_head_stats_bf16(&gs, nullptr, dummyf, dummyf, nullptr));                  // no ids
        EXPECT_ERR(umv_lm_head_stats_bf16(&gs, dummyl, nullptr, dummyf, nullptr));                  // no lse_partial
        EXPECT_ERR(umv_lm_head_stats_bf16(&gs, dummyl, dummyf, nullptr, nullptr));                  // no target_y
        gs.k_splits = 2;
        EXPECT_ERR(umv_lm_head_stats_bf16(&gs, dummyl, dummyf, dummyf, nullptr));                   // split-K
        gs.k_splits = 0; gs.epilogue = UMV_EPI_OUT_F32;
        EXPECT_ERR(umv_lm_head_stats_bf16(&gs, dummyl, dummyf, dummyf, nullptr));                   // an epilogue flag other than BIAS
        gs.epilogue = 0; gs.argmax_partial = (uint64_t*)dummyl;
        EXPECT_ERR(umv_lm_head_stats_bf16(&gs, dummyl, dummyf, dummyf, nullptr));                   // argmax_partial
        gs.argmax_partial = nullptr; gs.M = 0;
        EXPECT_OK(umv_lm_head_stats_bf16(&gs, dummyl, dummyf, dummyf, nullptr));                    // no rows
        EXPECT_ERR(umv_token_logprob_from_stats(nullptr, 9504, nullptr, nullptr, 152064, nullptr, 8, nullptr));
        EXPECT_ERR(umv_token_logprob_from_stats(dummyf, 4, dummyf, dummyl, 100, dummyf, 1, nullptr));   // 100 columns are not 4 tiles
        EXPECT_OK(umv_token_logprob_from_stats(dummyf, 4, dummyf, dummyl, 64, dummyf, 0, nullptr));     // no rows
    }
    EXPECT_ERR(umv_decode_top_logprobs(nullptr, 152064, 152064, nullptr, 9504, 0.f, nullptr, UMV_TOP_AFTER_LOGPROB, nullptr, nullptr, nullptr, 8,
                                       16, 5, nullptr, nullptr, nullptr, nullptr));
    EXPECT_ERR(umv_decode_top_logprobs(dummy16, 64, 64, dummyf, 4, 0.f, nullptr, UMV_TOP_AFTER_LOGPROB, dummyl, dummyl, nullptr, 1, 16, 0, dummyi,
                                       dummyf, dummyi, nullptr));                                 // n = 0
    EXPECT_ERR(umv_decode_top_logprobs(dummy16, 64, 64, dummyf, 4, 0.f, nullptr, UMV_TOP_AFTER_LOGPROB, dummyl, dummyl, nullptr, 1, 16,
                                       UMV_TOP_LOGPROBS_MAX + 1, dummyi, dummyf, dummyi, nullptr));
    EXPECT_ERR(umv_decode_top_logprobs(dummy16, 64, 64, dummyf, 4, 0.f, nullptr, UMV_TOP_AFTER_LOGPROB, dummyl, dummyl, nullptr, 1, 16, 5, dummyi,
                                       nullptr, dummyi, nullptr));                                // an output missing
    EXPECT_ERR(umv_decode_top_logprobs(dummy16, 64, 100, dummyf, 4, 0.f, nullptr, UMV_TOP_AFTER_LOGPROB, dummyl, dummyl, nullptr, 1, 16, 5, dummyi,
                                       dummyf, dummyi, nullptr));                                 // 100 columns are not 4 tiles
    EXPECT_ERR(umv_decode_top_logprobs(dummy16, 64, 64, dummyf, 4, 0.f, nullptr, 7, dummyl, dummyl, nullptr, 1, 16, 5, dummyi, dummyf, dummyi,
                                       nullptr));                                                 // no such step end
    EXPECT_OK(umv_decode_top_logprobs(dummy16, 64, 64, dummyf, 4, 0.f, nullptr, UMV_TOP_AFTER_TRUNCATED, dummyl, dummyl, nullptr, 0, 16, 5, dummyi,
                                      dummyf, dummyi, nullptr));                                  // no rows
    EXPECT_ERR(umv_top_logprobs_bf16(nullptr, 0, nullptr, 8, 152064, 0.f, 5, nullptr, nullptr, nullptr, nullptr));
    EXPECT_ERR(umv_top_logprobs_bf16(dummy16, 64, dummyl, 1, 64, 0.f, UMV_TOP_LOGPROBS_MAX + 1, dummyi, dummyf, dummyi, nullptr));
    EXPECT_ERR(umv_top_logprobs_bf16(dummy16, 12, dummyl, 1, 12, 0.f, 13, dummyi, dummyf, dummyi, nullptr));    // n > V
    EXPECT_ERR(umv_top_logprobs_bf16(dummy16, 64, dummyl, 1, 64, -1.f, 5, dummyi, dummyf, dummyi, nullptr));    // negative temperature
    EXPECT_OK(umv_top_logprobs_bf16(dummy16, 64, dummyl, 0, 64, 0.f, 5, dummyi, dummyf, dummyi, nullptr));      // no rows
    EXPECT_ERR(umv_sample_truncated_bf16(nullptr, 0, nullptr, 8, 152064, 1.0f, 1, nullptr, 50, 0.9f, 0.05f, nullptr, nullptr, nullptr));
    EXPECT_ERR(umv_sample_truncated_bf16(dummy16, 64, dummyl, 1, 64, 0.0f, 1, nullptr, 50, 0.9f, 0.f, nullptr, nullptr, nullptr));   // temperature 0
    EXPECT_ERR(umv_sample_truncated_bf16(dummy16, 64, dummyl, 1, 64, 1.0f, 1, nullptr, -1, 0.9f, 0.f, nullptr, nullptr, nullptr));   // top_k < 0
    EXPECT_ERR(umv_sample_truncated_bf16(dummy16, 64, dummyl, 1, 64, 1.0f, 1, nullptr, 0, 0.0f, 0.f, dummyf, dummyi, nullptr));      // top_p = 0
    EXPECT_ERR(umv_sample_truncated_bf16(dummy16, 64, dummyl, 1, 64, 1.0f, 1, nullptr, 0, 1.5f, 0.f, dummyf, dummyi, nullptr));      // top_p > 1
    EXPECT_ERR(umv_sample_truncated_bf16(dummy16, 64, dummyl, 1, 64, 1.0f, 1, nullptr, 5, 1.0f, 1.0f, dummyf, dummyi, nullptr));     // min_p = 1
    EXPECT_ERR(umv_sample_truncated_bf16(dummy16, 64, dummyl, 1, 64, 1.0f, 1, nullptr, 0, 1.0f, 0.f, dummyf, dummyi, nullptr));      // no filter on
    EXPECT_OK(umv_sample_truncated_bf16(dummy16, 64, dummyl, 0, 64, 1.0f, 1, nullptr, 5, 0.9f, 0.1f, dummyf, dummyi, nullptr));      // no rows
    EXPECT_ERR(umv_decode_step_end_truncated(nullptr, nullptr, nullptr, nullptr, nullptr, 9504, nullptr, nullptr, nullptr, nullptr, nullptr,
                                             152064, 152064, 1.f, nullptr, nullptr, 8, 16, 1, 50, 0.9f, 0.f, nullptr, nullptr, nullptr));
    EXPECT_ERR(umv_decode_step_end_truncated(dummyi, dummyi, dummyi, (const uint64_t*)dummyl, nullptr, 4, dummyl, dummyl, dummyl, dummyl, dummy16,
                                             64, 64, 1.f, nullptr, nullptr, 1, 16, 1, 0, 2.0f, 0.f, dummyf, dummyi, nullptr));   // top_p > 1
    EXPECT_ERR(umv_decode_step_end_truncated(dummyi, dummyi, dummyi, (const uint64_t*)dummyl, nullptr, 4, dummyl, dummyl, dummyl, dummyl, dummy16,
                                             64, 64, 1.f, nullptr, dummyf, 1, 16, 1, 5, 0.9f, 0.f, dummyf, dummyi, nullptr));    // logprob without lse_partial
    EXPECT_ERR(umv_decode_step_end_truncated(dummyi, dummyi, dummyi, (const uint64_t*)dummyl, nullptr, 4, dummyl, dummyl, dummyl, dummyl, dummy16,
                                             64, 64, 0.f, nullptr, nullptr, 1, 16, 1, 5, 0.9f, 0.f, dummyf, dummyi, nullptr));   // temperature 0
    EXPECT_OK(umv_decode_step_end_truncated(dummyi, dummyi, dummyi, (const uint64_t*)dummyl, nullptr, 4, dummyl, dummyl, dummyl, dummyl, dummy16,
                                            64, 64, 1.f, nullptr, nullptr, 0, 16, 1, 5, 0.9f, 0.f, dummyf, dummyi, nullptr));    // no samples
    // per-row sampling parameters
    alignas(16) umv_row_sampling rows[2];
    std::memset(rows, 0, sizeof rows);
    EXPECT_ERR(umv_decode_step_end_rows(nullptr, nullptr, nullptr, nullptr, nullptr, 9504, nullptr, nullptr, nullptr, nullptr, nullptr, 152064,
                                        152064, nullptr, nullptr, 8, 16, nullptr, nullptr, nullptr, nullptr));
    EXPECT_ERR(umv_decode_step_end_rows(dummyi, dummyi, dummyi, (const uint64_t*)dummyl, nullptr, 4, dummyl, dummyl, dummyl, dummyl, dummy16, 64,
                                        64, nullptr, nullptr, 1, 16, nullptr, dummyf, dummyi, nullptr));                 // no table
    EXPECT_ERR(umv_decode_step_end_rows(dummyi, dummyi, dummyi, (const uint64_t*)dummyl, nullptr, 4, dummyl, dummyl, dummyl, dummyl, dummy16, 64,
                                        64, nullptr, dummyf, 1, 16, rows, dummyf, dummyi, nullptr));                     // logprob without lse_partial
    EXPECT_ERR(umv_decode_step_end_rows(dummyi, dummyi, dummyi, (const uint64_t*)dummyl, nullptr, 3, dummyl, dummyl, dummyl, dummyl, dummy16, 64,
                                        64, nullptr, nullptr, 1, 16, rows, dummyf, dummyi, nullptr));                    // 64 columns are not 3 tiles
    EXPECT_OK(umv_decode_step_end_rows(dummyi, dummyi, dummyi, (const uint64_t*)dummyl, nullptr, 4, dummyl, dummyl, dummyl, dummyl, dummy16, 64,
                                       64, nullptr, nullptr, 0, 16, rows, dummyf, dummyi, nullptr));                     // no samples
    {
        umv_gemm_args gr;
        std::memset(&gr, 0, sizeof gr);
        gr.x = dummy16; gr.wp = dummy16; gr.out = dummy16; gr.ldx = 64; gr.ldo = 64; gr.M = 1; gr.N = 64; gr.K = 64;
        EXPECT_ERR(umv_gemm_bf16_rows(nullptr, rows, nullptr));
        EXPECT_ERR(umv_gemm_fp8w_rows(nullptr, rows, nullptr));
        EXPECT_ERR(umv_gemm_z13w_rows(nullptr, dummy8, rows, nullptr));
        EXPECT_ERR(umv_gemm_bf16_rows(&gr, rows, nullptr));      // the table without argmax_partial
        EXPECT_ERR(umv_gemm_fp8w_rows(&gr, rows, nullptr));
        EXPECT_ERR(umv_gemm_z13w_rows(&gr, dummy8, rows, nullptr));
        gr.argmax_partial = (uint64_t*)dummyl;
        EXPECT_ERR(umv_gemm_bf16_rows(&gr, nullptr, nullptr));   // no table
        gr.sample_temperature = 0.7f;                            // next to a scalar temperature
        EXPECT_ERR(umv_gemm_bf16_rows(&gr, rows, nullptr));
        EXPECT_ERR(umv_gemm_fp8w_rows(&gr, rows, nullptr));
        gr.sample_temperature = 0.f; gr.M = 65;                  // above 64 rows
        EXPECT_ERR(umv_gemm_bf16_rows(&gr, rows, nullptr));
        EXPECT_ERR(umv_gemm_z13w_rows(&gr, dummy8, rows, nullptr));
    }
    // logit penalties
    EXPECT_ERR(umv_logit_penalty_bf16(nullptr, nullptr));
    umv_logit_penalty_args lp;
    std::memset(&lp, 0, sizeof lp);
    EXPECT_ERR(umv_logit_penalty_bf16(&lp, nullptr));
    lp.logits = dummy16; lp.ld = 64; lp.ids = dummyl; lp.count = dummyi; lp.list = dummyi; lp.list_len = dummyi;
    lp.M = 1; lp.V = 64; lp.cap = 8; lp.n_static = 2; lp.repetition_penalty = 1.1f;
    lp.repetition_penalty = 0.f;                                 // r <= 0
    EXPECT_ERR(umv_logit_penalty_bf16(&lp, nullptr));
    lp.repetition_penalty = 1.1f; lp.presence_penalty = INFINITY;   // not finite
    EXPECT_ERR(umv_logit_penalty_bf16(&lp, nullptr));
    lp.presence_penalty = 0.f; lp.temperature = -1.f;            // negative temperature
    EXPECT_ERR(umv_logit_penalty_bf16(&lp, nullptr));
    lp.temperature = 0.f; lp.lse_partial = dummyf;               // lse_partial without argmax_partial
    EXPECT_ERR(umv_logit_penalty_bf16(&lp, nullptr));
    lp.lse_partial = nullptr; lp.n_static = 9;                   // cap below the static length
    EXPECT_ERR(umv_logit_penalty_bf16(&lp, nullptr));
    lp.n_static = 2; lp.argmax_partial = (uint64_t*)dummyl; lp.n_tiles = 3;     // 64 columns are not 3 tiles
    EXPECT_ERR(umv_logit_penalty_bf16(&lp, nullptr));
    lp.n_tiles = 4; lp.rows = rows;                              // non-neutral scalars (r = 1.1) next to the per-row table
    EXPECT_ERR(umv_logit_penalty_bf16(&lp, nullptr));
    lp.rows = nullptr; lp.M = 0;
    EXPECT_OK(umv_logit_penalty_bf16(&lp, nullptr));             // no rows
    // token automata: the mask and the state advance
    EXPECT_ERR(umv_logit_constrain_bf16(nullptr, nullptr));
    umv_logit_constrain_args lc;
    std::memset(&lc, 0, sizeof lc);
    EXPECT_ERR(umv_logit_constrain_bf16(&lc, nullptr));
    lc.logits = dummy16; lc.ld = 64; lc.M = 1; lc.V = 64; lc.state = dummyi;
    EXPECT_ERR(umv_logit_constrain_bf16(&lc, nullptr));          // no automaton
    lc.automaton.row_ptr = dummyi; lc.automaton.edge_token = dummyi; lc.automaton.edge_next = dummyi;
    lc.automaton.n_states = 0; lc.automaton.n_edges = 2;         // no state
    EXPECT_ERR(umv_logit_constrain_bf16(&lc, nullptr));
    lc.automaton.n_states = 1; lc.automaton.n_edges = -1;        // a negative edge count
    EXPECT_ERR(umv_logit_constrain_bf16(&lc, nullptr));
    lc.automaton.n_edges = 2; lc.automaton.edge_next = nullptr;  // edges without their next states
    EXPECT_ERR(umv_logit_constrain_bf16(&lc, nullptr));
    lc.automaton.edge_next = dummyi; lc.state = nullptr;         // no state words
    EXPECT_ERR(umv_logit_constrain_bf16(&lc, nullptr));
    lc.state = dummyi; lc.temperature = -1.f;                    // negative temperature
    EXPECT_ERR(umv_logit_constrain_bf16(&lc, nullptr));
    lc.temperature = 0.f; lc.lse_partial = dummyf;               // lse_partial without argmax_partial
    EXPECT_ERR(umv_logit_constrain_bf16(&lc, nullptr));
    lc.lse_partial = nullptr; lc.argmax_partial = (uint64_t*)dummyl; lc.n_tiles = 3;     // 64 columns are not 3 tiles
    EXPECT_ERR(umv_logit_constrain_bf16(&lc, nullptr));
    lc.n_tiles = 4; lc.ld = 32;                                  // a row stride below V
    EXPECT_ERR(umv_logit_constrain_bf16(&lc, nullptr));
    lc.ld = 64; lc.rows = rows; lc.temperature = 0.7f;           // a scalar temperature next to the per-row table
    EXPECT_ERR(umv_logit_constrain_bf16(&lc, nullptr));
    lc.rows = nullptr; lc.temperature = 0.f; lc.M = 0;
    EXPECT_OK(umv_logit_constrain_bf16(&lc, nullptr));           // no rows
    EXPECT_ERR(umv_constraint_advance(nullptr, dummyi, dummyl, 1, nullptr));
    EXPECT_ERR(umv_constraint_advance(&lc.automaton, nullptr, dummyl, 1, nullptr));
    EXPECT_ERR(umv_constraint_advance(&lc.automaton, dummyi, nullptr, 1, nullptr));
    EXPECT_ERR(umv_constraint_advance(&lc.automaton, dummyi, dummyl, -1, nullptr));
    lc.automaton.row_ptr = nullptr;
    EXPECT_ERR(umv_constraint_advance(&lc.automaton, dummyi, dummyl, 1, nullptr));
    lc.automaton.row_ptr = dummyi;
    EXPECT_OK(umv_constraint_advance(&lc.automaton, dummyi, dummyl, 0, nullptr));         // no rows
    // no-repeat n-grams
    EXPECT_ERR(umv_logit_ngram_ban_bf16(nullptr, nullptr));
    umv_ngram_ban_args ng;
    std::memset(&ng, 0, sizeof ng);
    EXPECT_ERR(umv_logit_ngram_ban_bf16(&ng, nullptr));
    ng.logits = dummy16; ng.ld = 64; ng.ids = dummyl; ng.hist = dummyi; ng.hist_ld = 8; ng.hist_len = dummyi; ng.M = 1; ng.V = 64; ng.n = 3;
    ng.hist = nullptr;                                           // no history
    EXPECT_ERR(umv_logit_ngram_ban_bf16(&ng, nullptr));
    ng.hist = dummyi; ng.hist_len = nullptr;                     // no length words
    EXPECT_ERR(umv_logit_ngram_ban_bf16(&ng, nullptr));
    ng.hist_len = dummyi; ng.ids = nullptr;                      // no fed tokens
    EXPECT_ERR(umv_logit_ngram_ban_bf16(&ng, nullptr));
    ng.ids = dummyl; ng.hist_ld = 0;                             // no room for a history
    EXPECT_ERR(umv_logit_ngram_ban_bf16(&ng, nullptr));
    ng.hist_ld = 8; ng.n = -1;                                   // a negative size
    EXPECT_ERR(umv_logit_ngram_ban_bf16(&ng, nullptr));
    ng.n = UMV_NGRAM_MAX + 1;                                    // a size above the maximum
    EXPECT_ERR(umv_logit_ngram_ban_bf16(&ng, nullptr));
    ng.n = 3; ng.temperature = -1.f;                             // negative temperature
    EXPECT_ERR(umv_logit_ngram_ban_bf16(&ng, nullptr));
    ng.temperature = 0.f; ng.lse_partial = dummyf;               // lse_partial without argmax_partial
    EXPECT_ERR(umv_logit_ngram_ban_bf16(&ng, nullptr));
    ng.lse_partial = nullptr; ng.argmax_partial = (uint64_t*)dummyl; ng.n_tiles = 3;     // 64 columns are not 3 tiles
    EXPECT_ERR(umv_logit_ngram_ban_bf16(&ng, nullptr));
    ng.n_tiles = 4; ng.ld = 32;                                  // a row stride below V
    EXPECT_ERR(umv_logit_ngram_ban_bf16(&ng, nullptr));
    ng.ld = 64; ng.rows = rows; ng.temperature = 0.7f;           // a scalar temperature next to the per-row table
    EXPECT_ERR(umv_logit_ngram_ban_bf16(&ng, nullptr));
    ng.rows = nullptr; ng.temperature = 0.f; ng.M = 0;
    EXPECT_OK(umv_logit_ngram_ban_bf16(&ng, nullptr));           // no rows
    // classifier-free guidance for text
    EXPECT_ERR(umv_logit_guidance_bf16(nullptr, nullptr));
    umv_logit_guidance_args lg;
    std::memset(&lg, 0, sizeof lg);
    EXPECT_ERR(umv_logit_guidance_bf16(&lg, nullptr));
    lg.logits = dummy16; lg.ld = 64; lg.M = 1; lg.V = 64; lg.pair = dummyi; lg.scale = dummyf; lg.log_beta = dummyf; lg.lse = dummyf;
    lg.row_max = dummyf; lg.stats = dummyf; lg.n_tiles = 4;
    lg.pair = nullptr;                                           // no pair table
    EXPECT_ERR(umv_logit_guidance_bf16(&lg, nullptr));
    lg.pair = dummyi; lg.lse = nullptr;                          // no lse words
    EXPECT_ERR(umv_logit_guidance_bf16(&lg, nullptr));
    lg.lse = dummyf; lg.temperature = -1.f;                      // negative temperature
    EXPECT_ERR(umv_logit_guidance_bf16(&lg, nullptr));
    lg.temperature = 0.f; lg.lse_partial = dummyf;               // lse_partial without argmax_partial
    EXPECT_ERR(umv_logit_guidance_bf16(&lg, nullptr));
    lg.lse_partial = nullptr; lg.n_tiles = 3;                    // 64 columns are not 3 tiles
    EXPECT_ERR(umv_logit_guidance_bf16(&lg, nullptr));
    lg.n_tiles = 4; lg.ld = 32;                                  // a row stride below V
    EXPECT_ERR(umv_logit_guidance_bf16(&lg, nullptr));
    lg.ld = 64; lg.stats = nullptr;                              // no statistics that serve and no workspace
    EXPECT_ERR(umv_logit_guidance_bf16(&lg, nullptr));
    lg.stats = dummyf; lg.M = 65536;                             // too many rows
    EXPECT_ERR(umv_logit_guidance_bf16(&lg, nullptr));
    lg.M = 0;
    EXPECT_OK(umv_logit_guidance_bf16(&lg, nullptr));            // no rows
    EXPECT_ERR(umv_guidance_feed(nullptr, dummyl, dummyl, dummyl, dummyl, 1, 4, nullptr));
    EXPECT_ERR(umv_guidance_feed(dummyi, nullptr, dummyl, dummyl, dummyl, 1, 4, nullptr));
    EXPECT_ERR(umv_guidance_feed(dummyi, dummyl, dummyl, dummyl, nullptr, 1, 4, nullptr));
    EXPECT_ERR(umv_guidance_feed(dummyi, dummyl, dummyl, dummyl, dummyl, -1, 4, nullptr));
    EXPECT_OK(umv_guidance_feed(dummyi, dummyl, dummyl, dummyl, dummyl, 0, 4, nullptr));          // no rows
    // beam search decode
    alignas(16) static int32_t beam_words[8];
    EXPECT_ERR(umv_beam_candidates(nullptr, 64, 64, dummyf, 4, 1, 4, dummyi, dummyf, dummyi, nullptr));
    EXPECT_ERR(umv_beam_candidates(dummy16, 64, 64, nullptr, 4, 1, 4, dummyi, dummyf, dummyi, nullptr));          // no statistics
    EXPECT_ERR(umv_beam_candidates(dummy16, 64, 64, dummyf, 4, 1, 4, nullptr, dummyf, dummyi, nullptr));          // no id list
    EXPECT_ERR(umv_beam_candidates(dummy16, 64, 64, dummyf, 4, 1, 5, dummyi, dummyf, dummyi, nullptr));           // 2K is even
    EXPECT_ERR(umv_beam_candidates(dummy16, 64, 64, dummyf, 4, 1, 22, dummyi, dummyf, dummyi, nullptr));          // K above the maximum
    EXPECT_ERR(umv_beam_candidates(dummy16, 64, 4, dummyf, 1, 1, 4, dummyi, dummyf, dummyi, nullptr));            // V must exceed 2K
    EXPECT_ERR(umv_beam_candidates(dummy16, 64, 64, dummyf, 3, 1, 4, dummyi, dummyf, dummyi, nullptr));           // 64 columns are not 3 tiles
    EXPECT_OK(umv_beam_candidates(dummy16, 64, 64, dummyf, 4, 0, 4, dummyi, dummyf, dummyi, nullptr));            // no rows
    EXPECT_ERR(umv_beam_step_end(nullptr, nullptr));
    umv_beam_step_args bs;
    std::memset(&bs, 0, sizeof bs);
    EXPECT_ERR(umv_beam_step_end(&bs, nullptr));
    bs.tok_slot = dummyi; bs.tok_pos = dummyi; bs.kv_len = dummyi; bs.ids = dummyl; bs.step_idx = dummyl; bs.cand_ids = dummyi;
    bs.cand_lp = dummyf; bs.scores = dummyf; bs.beam_tok = dummyi; bs.beam_parent = dummyi; bs.beam_lp = dummyf; bs.fin_f = dummyf;
    bs.fin_i = dummyi; bs.hdr = beam_words; bs.len_norm = dummyf; bs.table = dummyi; bs.own = dummyi; bs.j0 = dummyi; bs.copies = beam_words + 4;
    bs.table_stride = 8; bs.n_own = 2; bs.B = 0; bs.K = 3; bs.max_len = 4; bs.end_token_id = -1;
    EXPECT_OK(umv_beam_step_end(&bs, nullptr));                  // no requests
    bs.K = 0;
    EXPECT_ERR(umv_beam_step_end(&bs, nullptr));
    bs.K = UMV_BEAM_K_MAX + 1;
    EXPECT_ERR(umv_beam_step_end(&bs, nullptr));
    bs.K = 3; bs.n_own = UMV_BEAM_TABLE_ENTRIES;                 // K * n_own above what a workgroup carries
    EXPECT_ERR(umv_beam_step_end(&bs, nullptr));
    bs.n_own = 2; bs.copies = beam_words + 1;                    // misaligned copy list
    EXPECT_ERR(umv_beam_step_end(&bs, nullptr));
    bs.copies = beam_words + 4; bs.own = nullptr;
    EXPECT_ERR(umv_beam_step_end(&bs, nullptr));
    const void* beam_pools[2] = {dummy16, dummy16};
    EXPECT_ERR(umv_beam_kv_copy(nullptr, beam_pools, 0, 1, 2, 128, 4, 1, nullptr));
    EXPECT_ERR(umv_beam_kv_copy(beam_words, nullptr, 0, 1, 2, 128, 4, 1, nullptr));
    EXPECT_ERR(umv_beam_kv_copy(beam_words, beam_pools, 0, 1, 2, 100, 4, 1, nullptr));    // hd is a multiple of 8
    EXPECT_ERR(umv_beam_kv_copy(beam_words, beam_pools, 0, 1, 2, 128, 4, 0, nullptr));    // no chunks
    EXPECT_ERR(umv_beam_kv_copy(beam_words + 1, beam_pools, 0, 1, 2, 128, 4, 1, nullptr));   // misaligned copy list
    EXPECT_OK(umv_beam_kv_copy(beam_words, beam_pools, 0, 1, 2, 128, 4, 1, nullptr));     // no rows
    // banned sequences
    EXPECT_ERR(umv_logit_sequence_ban_bf16(nullptr, nullptr));
    umv_sequence_ban_args sq;
    std::memset(&sq, 0, sizeof sq);
    EXPECT_ERR(umv_logit_sequence_ban_bf16(&sq, nullptr));
    sq.logits = dummy16; sq.ld = 64; sq.ids = dummyl; sq.seq_ptr = dummyi; sq.seq_tok = dummyi; sq.seq_until = dummyi; sq.tail = dummyi;
    sq.count = dummyi; sq.M = 1; sq.V = 64; sq.S = 1; sq.n_tok = 2; sq.max_m = 2;
    sq.S = -1;                                                   // a negative entry count
    EXPECT_ERR(umv_logit_sequence_ban_bf16(&sq, nullptr));
    sq.S = UMV_SEQ_ENTRIES_MAX + 1; sq.n_tok = sq.S;             // more entries than the maximum
    EXPECT_ERR(umv_logit_sequence_ban_bf16(&sq, nullptr));
    sq.S = 1; sq.n_tok = 2; sq.seq_ptr = nullptr;                // entries without a table
    EXPECT_ERR(umv_logit_sequence_ban_bf16(&sq, nullptr));
    sq.seq_ptr = dummyi; sq.seq_until = nullptr;
    EXPECT_ERR(umv_logit_sequence_ban_bf16(&sq, nullptr));
    sq.seq_until = dummyi; sq.n_tok = UMV_SEQ_MAX + 1;           // more tokens than S entries can hold
    EXPECT_ERR(umv_logit_sequence_ban_bf16(&sq, nullptr));
    sq.n_tok = 2; sq.max_m = UMV_SEQ_MAX + 1;                    // a longest entry above the maximum
    EXPECT_ERR(umv_logit_sequence_ban_bf16(&sq, nullptr));
    sq.max_m = 2; sq.ids = nullptr;                              // no fed tokens
    EXPECT_ERR(umv_logit_sequence_ban_bf16(&sq, nullptr));
    sq.ids = dummyl; sq.tail = nullptr;                          // the plain form without its tail
    EXPECT_ERR(umv_logit_sequence_ban_bf16(&sq, nullptr));
    sq.tail = dummyi; sq.count = nullptr;
    EXPECT_ERR(umv_logit_sequence_ban_bf16(&sq, nullptr));
    sq.count = dummyi; sq.K = 2; sq.M = 2; sq.max_len = 4;       // the beam form without its back-pointers
    EXPECT_ERR(umv_logit_sequence_ban_bf16(&sq, nullptr));
    sq.beam_tok = dummyi; sq.beam_parent = dummyi; sq.step_idx = dummyl; sq.start_ids = dummyl; sq.K = UMV_BEAM_K_MAX + 1;
    EXPECT_ERR(umv_logit_sequence_ban_bf16(&sq, nullptr));       // K above the maximum
    sq.K = 2; sq.M = 3;                                          // rows that are no multiple of K
    EXPECT_ERR(umv_logit_sequence_ban_bf16(&sq, nullptr));
    sq.M = 2; sq.rows = rows; sq.argmax_partial = (uint64_t*)dummyl; sq.n_tiles = 4;      // the beam form is greedy
    EXPECT_ERR(umv_logit_sequence_ban_bf16(&sq, nullptr));
    sq.rows = nullptr; sq.argmax_partial = nullptr; sq.n_tiles = 0; sq.K = 0; sq.M = 1; sq.temperature = -1.f;   // negative temperature
    EXPECT_ERR(umv_logit_sequence_ban_bf16(&sq, nullptr));
    sq.temperature = 0.f; sq.lse_partial = dummyf;               // lse_partial without argmax_partial
    EXPECT_ERR(umv_logit_sequence_ban_bf16(&sq, nullptr));
    sq.lse_partial = nullptr; sq.argmax_partial = (uint64_t*)dummyl; sq.n_tiles = 3;     // 64 columns are not 3 tiles
    EXPECT_ERR(umv_logit_sequence_ban_bf16(&sq, nullptr));
    sq.n_tiles = 4; sq.ld = 32;                                  // a row stride below V
    EXPECT_ERR(umv_logit_sequence_ban_bf16(&sq, nullptr));
    sq.ld = 64; sq.M = 0;
    EXPECT_OK(umv_logit_sequence_ban_bf16(&sq, nullptr));        // no rows
    sq.S = 0; sq.n_tok = 0; sq.max_m = 0; sq.seq_ptr = nullptr; sq.seq_tok = nullptr; sq.seq_until = nullptr;
    EXPECT_OK(umv_logit_sequence_ban_bf16(&sq, nullptr));        // an empty table records only
    // speculative step end
    EXPECT_ERR(umv_decode_step_end_speculative(nullptr, nullptr));
    umv_spec_step_args sp;
    std::memset(&sp, 0, sizeof sp);
    EXPECT_ERR(umv_decode_step_end_speculative(&sp, nullptr));
    sp.tok_slot = dummyi; sp.tok_pos = dummyi; sp.kv_len = dummyi; sp.argmax_partial = (const uint64_t*)dummyl; sp.n_tiles = 4; sp.V = 64;
    sp.ids = dummyl; sp.out_ids = dummyl; sp.out_ld = 8; sp.n_out = dummyi; sp.limit = dummyi; sp.n_draft = dummyi; sp.hist = dummyi;
    sp.hist_ld = 8; sp.hist_len = dummyi; sp.stats = dummyi; sp.B = 1; sp.k = 0; sp.ngram_min = 2; sp.ngram_max = 4;
    EXPECT_ERR(umv_decode_step_end_speculative(&sp, nullptr));   // k < 1
    sp.k = 3; sp.B = 17;                                          // 68 rows
    EXPECT_ERR(umv_decode_step_end_speculative(&sp, nullptr));
    sp.B = 1; sp.ngram_min = 0;
    EXPECT_ERR(umv_decode_step_end_speculative(&sp, nullptr));
    sp.ngram_min = 5;                                             // above ngram_max
    EXPECT_ERR(umv_decode_step_end_speculative(&sp, nullptr));
    sp.ngram_min = 2; sp.stats = nullptr;
    EXPECT_ERR(umv_decode_step_end_speculative(&sp, nullptr));
    sp.stats = dummyi; sp.predicted = dummyl;                     // predicted without pred_len
    EXPECT_ERR(umv_decode_step_end_speculative(&sp, nullptr));
    sp.predicted = nullptr; sp.n_tiles = 3;                       // 64 columns are not 3 tiles
    EXPECT_ERR(umv_decode_step_end_speculative(&sp, nullptr));
    sp.n_tiles = 4; sp.B = 0;
    EXPECT_OK(umv_decode_step_end_speculative(&sp, nullptr));    // no samples
    // sampled speculative step end: the pick launch and the commit launch
    EXPECT_ERR(umv_decode_pick_rows(nullptr, nullptr, 4, nullptr, 64, 64, nullptr, 1, nullptr, nullptr, nullptr, nullptr, nullptr));
    EXPECT_ERR(umv_decode_pick_rows((const uint64_t*)dummyl, nullptr, 4, dummy16, 64, 64, nullptr, 1, dummyl, nullptr, dummyf, dummyi,
                                    nullptr));                                                                  // no table
    EXPECT_ERR(umv_decode_pick_rows((const uint64_t*)dummyl, nullptr, 4, dummy16, 64, 64, rows, 1, dummyl, dummyf, dummyf, dummyi,
                                    nullptr));                                                                  // logprob without lse_partial
    EXPECT_ERR(umv_decode_pick_rows((const uint64_t*)dummyl, nullptr, 3, dummy16, 64, 64, rows, 1, dummyl, nullptr, dummyf, dummyi,
                                    nullptr));                                                                  // 64 columns are not 3 tiles
    EXPECT_ERR(umv_decode_pick_rows((const uint64_t*)dummyl, nullptr, 4, dummy16, 64, 64, rows, 65, dummyl, nullptr, dummyf, dummyi,
                                    nullptr));                                                                  // 65 rows
    EXPECT_OK(umv_decode_pick_rows((const uint64_t*)dummyl, nullptr, 4, dummy16, 64, 64, rows, 0, dummyl, nullptr, dummyf, dummyi,
                                   nullptr));                                                                   // no rows
    EXPECT_ERR(umv_decode_step_end_speculative_rows(nullptr, nullptr));
    umv_spec_rows_step_args sr;
    std::memset(&sr, 0, sizeof sr);
    EXPECT_ERR(umv_decode_step_end_speculative_rows(&sr, nullptr));
    sr.step = sp; sr.step.B = 1; sr.step.argmax_partial = nullptr;       // the keys are not read
    sr.picks = dummyl;
    EXPECT_ERR(umv_decode_step_end_speculative_rows(&sr, nullptr));     // no table
    sr.rows = rows; sr.picks = nullptr;
    EXPECT_ERR(umv_decode_step_end_speculative_rows(&sr, nullptr));     // no picks
    sr.picks = dummyl; sr.row_logprob = dummyf;                          // row_logprob without out_logprobs
    EXPECT_ERR(umv_decode_step_end_speculative_rows(&sr, nullptr));
    sr.row_logprob = nullptr; sr.step.k = 64;                            // 65 rows
    EXPECT_ERR(umv_decode_step_end_speculative_rows(&sr, nullptr));
    sr.step.k = 3; sr.step.B = 0;
    EXPECT_OK(umv_decode_step_end_speculative_rows(&sr, nullptr));      // no samples
    EXPECT_ERR(umv_timestep_embed(nullptr, nullptr, nullptr, 4, 128, nullptr));
    EXPECT_ERR(umv_cfg_renorm_euler(nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 1, 4.0f, 1.5f, 0.f, 0, 0.1f, 64, nullptr));
    // VAE
    EXPECT_ERR(umv_conv2d_nhwc_bf16(nullptr, nullptr, nullptr, nullptr, nullptr, 1, 128, 32, 32, 128, 3, 0, nullptr));
    EXPECT_ERR(umv_conv2d_nhwc_bf16(dummy16, dummy16, nullptr, nullptr, dummy16, 1, 128, 32, 32, 128, 5, 0, nullptr));   // 5 x 5
    EXPECT_ERR(umv_conv2d_nhwc_bf16(dummy16, dummy16, nullptr, nullptr, dummy16, 1, 128, 32, 32, 128, 1, 1, nullptr));   // 1 x 1 upsample
    EXPECT_ERR(umv_conv2d_nhwc_bf16(dummy16, dummy16, nullptr, nullptr, dummy16, 1, 128, 32, 32, 128, 1, 2, nullptr));   // 1 x 1 downsample
    EXPECT_ERR(umv_conv2d_nhwc_bf16(dummy16, dummy16, nullptr, nullptr, dummy16, -1, 128, -32, 32, 128, 3, 0, nullptr));
    EXPECT_ERR(umv_conv2d_nhwc_bf16(dummy16, dummy16, nullptr, nullptr, dummy16, 1, 128, 32, 32, 0, 3, 0, nullptr));
    EXPECT_OK(umv_conv2d_nhwc_bf16(dummy16, dummy16, nullptr, nullptr, dummy16, 1, 128, 1, 32, 128, 3, 2, nullptr));     // one row: empty
    EXPECT_ERR(umv_groupnorm_nhwc_bf16(nullptr, nullptr, nullptr, nullptr, nullptr, 1, 1024, 128, 1e-6f, 1, nullptr));
    EXPECT_ERR(umv_nchw_f32_to_nhwc_bf16(nullptr, nullptr, 1, 3, 32, 32, 8, nullptr));
    EXPECT_ERR(umv_unpatchify_latent(nullptr, nullptr, 16, 16, 2, 16, 0.36f, 0.11f, nullptr));
    EXPECT_ERR(umv_pixels_to_u8(nullptr, nullptr, 1024, 8, nullptr));
    EXPECT_ERR(umv_softmax_rows_f32(nullptr, 0, nullptr, 0, nullptr, 16, 1024, 1.0f, nullptr));
    EXPECT_ERR(umv_softmax_rows_f32(dummyf, 1025, dummy16, 1025, dummyf, 1, 1025, 1.0f, nullptr));   // odd n
    EXPECT_ERR(umv_rowscale_f32_bf16(nullptr, 0, nullptr, nullptr, 0, 16, 512, nullptr));
    EXPECT_ERR(umv_latent_sample_patchify(nullptr, nullptr, nullptr, 0, 56, 56, 16, 28, 28, 2, 0.36f, 0.11f, nullptr));
    (void)dummy8;
}

int main(int argc, char** argv) {
    const int threads = argc > 1 ? std::atoi(argv[1]) : 8, rounds = argc > 2 ? std::atoi(argv[2]) : 200;
    queries();
    bad_arguments();
    std::printf("single thread: %d failure(s)\n", failures.load());
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; ++t)
        pool.emplace_back([rounds] {
            for (int r = 0; r < rounds; ++r) { queries(); bad_arguments(); }
        });
    for (auto& th : pool) th.join();
    std::printf("%d threads x %d rounds: %d failure(s) in all\n", threads, rounds, failures.load());
    return failures.load() ? 1 : 0;
}
