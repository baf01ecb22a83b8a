/*
 * libunimedvl_hip.so - C ABI of the MI355X (gfx950) kernel library that replaces the
 * third-party native ops on UniMedVL's forward path (SURVEY.md section 2.2 / 8b "B2").
 *
 * The reference has no FFI of its own: its native work is reached through
 * flash_attn / torch.nn.functional calls from Python.  Each entry point below names
 * the reference call site(s) it stands in for (paths relative to
 * /root/reference/codes/).  All pointers are DEVICE pointers owned by the caller;
 * nothing here allocates persistent memory; every call is asynchronous on `stream`
 * (a hipStream_t passed as void*).  Return 0 on success, negative on error
 * (message from umv_last_error()); nothing throws across the ABI.
 *
 * bf16 tensors are uint16_t bit patterns.  "rows" are tokens (packed NaViT
 * sequences have no batch dimension, as in the reference).
 */
#ifndef UNIMEDVL_HIP_H
#define UNIMEDVL_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* umv_stream_t;

int umv_version(void);
const char* umv_last_error(void);

/* ------------------------------------------------------------------ weights
 * nn.Linear weights [N,K] (row-major, modeling_qwen2.py:283-286, 229-231) are
 * re-tiled ONCE at load time into MFMA A-fragment order:
 *   P[n/16][k/32][lane = ((k%32)/8)*16 + n%16][k%8], zero padded to N%16==0, K%32==0
 * so that a wavefront streams 1 KiB contiguous per 16x32 tile. */
size_t umv_packed_weight_elems(int N, int K);
int umv_pack_weight_bf16(const uint16_t* w, uint16_t* packed, int N, int K, umv_stream_t stream);
/* Decode-only second copy with `th`-row tiles, Q[n/th][k/32][(k%32)/8][n%th][k%8], built from the standard
 * image: with th = N/256 (14 for N=3584, 9 for N=4608) the weight-streaming GEMM has exactly one (or two)
 * tiles per CU of the 256-CU chip instead of 224-288 16-row tiles. */
size_t umv_repacked_weight_elems(int N, int K, int th);
int umv_repack_weight_rows_bf16(const uint16_t* packed16, uint16_t* out, int N, int K, int th, umv_stream_t stream);
/* gate_proj / up_proj [I,K] each -> one packed [2I,K] with 16-row tiles interleaved
 * (gate tile t, up tile t, ...) so SwiGLU fuses into the GEMM epilogue. */
int umv_pack_weight_swiglu_bf16(const uint16_t* gate, const uint16_t* up, uint16_t* packed, int I, int K,
                                umv_stream_t stream);

/* ------------------------------------------------------------------ GEMM
 * out[m,n] = epilogue(sum_k x[m,k] * W[n,k]); fp32 accumulate on MFMA; replaces
 * F.linear at qwen2_navit.py:541-543,555-562,617-620, modeling_qwen2.py:234-235,
 * bagel.py:1295,1104,1133, siglip_navit.py:190,216-218,243,256-258,
 * modeling_utils.py:108,120-122.  Epilogue order (each step rounds to bf16 exactly
 * where the reference's bf16 tensors are materialised):
 *   v = acc (+bias) -> bf16 ; GELU_TANH / SILU -> bf16 ; SWIGLU: bf16(bf16(silu(g))*u) ;
 *   RESIDUAL: bf16(v + residual[m,n])
 * Values: every add is one fp32 addition (denormals kept) rounded to nearest even; bf16 subnormal weights and
 * activations take part in the product.  GELU_TANH (torch's approximate="tanh") and SILU are x / (1 + 2^t) on the
 * hardware exp2 / rcp: at most one bf16 value from the exact function; where 1 / (1 + 2^t) is below 2^-126 (SiLU:
 * x <= -87.5, GELU: x <= -10.0625, and |x| < 2^-126) the result may be flushed to zero - the left tails give -0.
 * +inf -> +inf, -inf -> NaN (x * 0, as torch on the device), NaN -> NaN. */
enum {
    UMV_EPI_BIAS = 1,
    UMV_EPI_GELU_TANH = 2,
    UMV_EPI_SILU = 4,
    UMV_EPI_RESIDUAL = 8,
    UMV_EPI_SWIGLU = 16, /* packed weight from umv_pack_weight_swiglu_bf16; out is [M, N/2] */
    UMV_EPI_OUT_F32 = 32 /* store raw fp32 accumulators (+bias), no rounding */
};
/* Per-row sampling parameters of a decode step: one element per row, in DEVICE memory, 16-byte aligned, 48 bytes:
 *   offset 0 seed, 8 draw, 16 stream, 20 temperature, 24 top_k, 28 top_p, 32 min_p, 36 repetition_penalty, 40 presence_penalty,
 *   44 frequency_penalty.
 * Read by the lm_head epilogue (umv_gemm_bf16_rows / _z13w_rows / _fp8w_rows), umv_logit_penalty_bf16 (rows) and umv_decode_step_end_rows; the semantics
 * are spelled out under "per-row sampling parameters" below.  The entries cannot look into device memory: the CALLER guarantees
 * temperature finite (any value <= 0 marks a greedy row), and on a sampled row top_k >= 0, top_p in (0, 1], min_p in [0, 1); on every
 * row repetition_penalty finite and > 0, presence_penalty and frequency_penalty finite; draw >= 0. */
typedef struct {
    uint64_t seed;        /* the request's seed */
    int64_t  draw;        /* the request's own draw counter: takes the place of *sample_step in the key; the step end adds 1 */
    uint32_t stream;      /* takes the place of the row index m in the key */
    float    temperature; /* > 0: sample; anything else (0, negative, NaN): a greedy row, and the row's filters are ignored */
    int32_t  top_k;       /* 0 = off */
    float    top_p;       /* 1 = off */
    float    min_p;       /* 0 = off */
    float    repetition_penalty, presence_penalty, frequency_penalty;   /* 1 / 0 / 0 = off */
} umv_row_sampling;
typedef struct {
    const uint16_t* x;        /* [M,K] bf16, row stride ldx (elements), K%8==0 */
    int64_t ldx;
    const uint16_t* wp;       /* packed weight */
    const uint16_t* bias;     /* [N] or NULL */
    const uint16_t* residual; /* [M,N] row stride ldr, or NULL */
    int64_t ldr;
    void* out;                /* bf16 (or fp32) [M,N'] row stride ldo */
    int64_t ldo;
    const int32_t* row_idx;   /* optional [M]: x, residual and out rows are row_idx[m] (MoT routing,
                                 qwen2_navit.py:552-562,619-620,891-898) */
    int M, N, K;
    int epilogue;
    const uint16_t* norm_w;   /* optional [K]: fuse Qwen2RMSNorm(x) * norm_w into the prologue (decode path,
                                 qwen2_navit.py:861,888,1164 feeding :541-543, modeling_qwen2.py:234, bagel.py:1295);
                                 needs M <= 16 and K <= 4096 */
    float norm_eps;
    int tile_rows;            /* rows per n-tile of `wp`: 0 or 16 = umv_pack_weight_bf16 image; 1..15 = an image made by
                                 umv_repack_weight_rows_bf16 (decode only, M <= 64) */
    const float* w_scale;     /* umv_gemm_fp8w only: per-channel scales written by umv_quantize_pack_weight_fp8 */
    int k_splits;             /* > 1 (umv_gemm_bf16, M <= 64, 16-row image, no SwiGLU / norm_w): split-K decode mode. K is cut
                                 into k_splits ranges; `out` is then an fp32 buffer [k_splits][rows][ldo] (split s at
                                 out + s*split_stride) of RAW partial sums - no bias, activation or residual: the consumer
                                 (umv_qkv_post partials input, umv_residual_rmsnorm_bf16) adds the splits in order 0..S-1 and
                                 finishes the row with the reference's roundings */
    int64_t split_stride;     /* elements between consecutive splits of `out` */
    uint64_t* argmax_partial; /* optional [M][ceil(N/16)] (M <= 64, bf16 out, plain 16-row image): greedy argmax as an epilogue of
                                 the lm_head GEMM (bagel.py:1295-1301).  Every 16-column tile writes one key per row:
                                 (order-preserving image of the stored bf16 logit) << 32 | (0xFFFFFFFF - column); the maximum
                                 key over a row is torch.argmax(logits) (lowest index on ties, NaN highest).  Finished by
                                 umv_decode_step_end_argmax.  The logits are still written to `out`. */
    int64_t x_rows;           /* with row_idx: number of rows of the buffer `x` points into (rows row_idx may name), 0 = unknown.
                                 The 4-wave tiles of the M > 64 path address x through 32-bit offsets and take a row-indexed call
                                 only when x_rows * ldx * 2 < 2 GiB is known; unknown keeps the 8-wave tiles (same results). */
    float sample_temperature; /* with argmax_partial, > 0: the keys are those of SAMPLING instead of greedy decoding (bagel.py:1297-1299:
                                 probs = softmax(logits / temperature), token = multinomial(probs, 1)) by the Gumbel-max rule: the key of
                                 column n orders bf16(logit / T) - ln(-ln(u)), u uniform in (0, 1] from a counter-based generator
                                 (splitmix64 of sample_seed, *sample_step, the row and n - the stream of umv_sample_bf16), so the maximum key
                                 over a row is one draw from the softmax.  0: greedy keys. */
    uint64_t sample_seed;
    const int64_t* sample_step; /* device word: the decode step (changes the draw every step under a replayed HIP graph); NULL = 0 */
    float* lse_partial;       /* optional [M][ceil(N/16)][2] fp32, only together with argmax_partial (UMV_ERR_ARG otherwise): the softmax
                                 statistics of every 16-column tile of a row for the token log-probability (see "token log-probabilities"
                                 below).  With y[n] the value the token pick orders WITHOUT noise - the stored bf16 logit when
                                 sample_temperature == 0, bf16(logit / T) when it is > 0 - entry [m][t] = (m_t, s_t): m_t = max of y over
                                 the tile's valid columns, s_t = sum of exp(y - m_t) over them (a -inf column adds 0; a tile of -inf only
                                 is (-inf, 0), never NaN; a NaN column makes s_t NaN).  Fixed order - the lane's four columns, then the
                                 row's four lane groups as a tree - so the bits do not depend on M or on the workgroup.  Keys and logits
                                 are the bits of the same call without it.  Finished by umv_decode_step_end_logprob. */
} umv_gemm_args;
int umv_gemm_bf16(const umv_gemm_args* a, umv_stream_t stream);
/* The lm_head call with a per-row sampling table (see "per-row sampling parameters"; umv_gemm_fp8w_rows and umv_gemm_z13w_rows are the
 * same for the other two images that carry argmax_partial): rows [M], device memory, 16-byte aligned, read only.  Row m takes its
 * temperature and the (seed, draw, stream) of its sampling key from rows[m] instead of sample_temperature / sample_seed / *sample_step /
 * m - greedy and sampled rows in one call.  UMV_ERR_ARG without rows, without argmax_partial, above 64 rows or with
 * sample_temperature != 0; everything else as the entry without the table, whose struct - and so every kernel argument - is unchanged. */
int umv_gemm_bf16_rows(const umv_gemm_args* a, const umv_row_sampling* rows, umv_stream_t stream);
/* Host-only query: the tiled-kernel configuration umv_gemm_bf16 picks for an M x N x K problem (0 for M <= 64, the
 * weight-streaming kernels; 266 = 256x256x32 interleaved, 268 = 256(n)x128(m), 384 = 384(n)x128(m), 270 = 128x128,
 * 64 = 128(n)x64(m)x64).
 * Lets the parity tests assert that a shape reaches the kernel variant it is meant to pin. */
int umv_gemm_tile_config(int M, int N, int K);

/* ------------------------------------------------------------------ fp8 weights (BASELINE.json configs[4]; no
 * reference counterpart: the reference only has bf16 weights, qwen2_navit.py:541-562 / modeling_qwen2.py:229-235)
 * Weight-only OCP e4m3 with one POWER-OF-TWO scale per output channel, s[n] = the smallest 2^e with
 * 448 * 2^e >= max_k |W[n,k]|, q = rne_e4m3(W / s).  W' = q * s is exact in bf16, so
 *   umv_gemm_fp8w(x, q, s)  ==  umv_gemm_bf16(x, pack(W'))   bit for bit   (K % 512 == 0)
 * and prefill / diffusion (M > 64) run umv_gemm_bf16 on the bf16 image of W' while decode streams half the bytes.
 * Image: P8[n/16][k/64][lane = ((k%32)/8)*16 + n%16][(k%64)/32][k%8] bytes, zero padded; `scale` is f32
 * [ceil(N/16)*16] in image row order.  With w_up != NULL, `w`/`w_up` are gate_proj / up_proj [rows=I, K] and the
 * image interleaves their 16-row tiles (UMV_EPI_SWIGLU).  deq / deq_up (optional) receive W' row-major. */
size_t umv_packed_weight_fp8_bytes(int N, int K);
int umv_quantize_pack_weight_fp8(const uint16_t* w, const uint16_t* w_up, uint8_t* packed8, float* scale, uint16_t* deq,
                                 uint16_t* deq_up, int rows, int K, umv_stream_t stream);
/* M <= 64 only; a->wp = the e4m3 image, a->w_scale = its scales; norm_w / tile_rows unsupported */
int umv_gemm_fp8w(const umv_gemm_args* a, umv_stream_t stream);
int umv_gemm_fp8w_rows(const umv_gemm_args* a, const umv_row_sampling* rows, umv_stream_t stream);   /* see umv_gemm_bf16_rows */

/* ------------------------------------------------------------------ MXFP4 weights (llm_weight_dtype = "fp4"; no reference
 * counterpart).  Weight-only e2m1 with one E8M0 power-of-two scale per BLOCK of 32 consecutive k of a row (K % 32 == 0):
 *   s = 2^e, e = the smallest integer with 6 * 2^e >= max|W[block]| (no clipping; the OCP MX rule, which saturates, is not used),
 *   clamped to [-127, 127], e = 0 for an all-zero block, stored as the byte e + 127;
 *   q = rne_e2m1(W / s) (ties to the even code), the SIGN KEPT: a negative value that rounds to zero is code 8 (-0).
 * W' = q * s is exact in bf16, so
 *   umv_gemm_mxfp4w(x, img)  ==  umv_gemm_bf16(x, pack(W'))   bit for bit   (K % 512 == 0, no split-K, wherever umv_gemm_bf16
 *                                                                         takes its weight-streaming kernel: not SwiGLU at 33..64
 *                                                                         rows with K >= 1024, which it runs on a tiled kernel)
 * Image (umv_packed_weight_mxfp4_bytes; NP = ceil(ceil(N/16) / 2) pairs of 16-row tiles, KT8 = ceil(K/64)):
 *   codes  C[p][k/64][lane = ((k%32)/8)*16 + n%16][16 B] at byte 0: bytes 0..3 tile 2p k%64 < 32, 4..7 tile 2p k%64 >= 32,
 *          8..11 tile 2p+1 k%64 < 32, 12..15 tile 2p+1 k%64 >= 32; element k%8 is nibble k%8 of its 4 bytes, low nibble first;
 *   scales S[p][k/64][n%16][4 B] at byte NP*KT8*1024, in the same (tile, k half) order as the code words.
 * Padding is code 0 with scale byte 127.  With w_up != NULL, `w`/`w_up` are gate_proj / up_proj [rows=I, K] and the image
 * interleaves their 16-row tiles (UMV_EPI_SWIGLU), so pair t is (gate tile t, up tile t).  deq / deq_up (optional) receive W'
 * row-major.  All buffers 16-byte aligned, K <= 65536; weights finite with |W| < 1.75 * 2^127 (from there W' leaves bf16). */
size_t umv_packed_weight_mxfp4_bytes(int N, int K);
int umv_quantize_pack_weight_mxfp4(const uint16_t* w, const uint16_t* w_up, uint8_t* packed4, uint16_t* deq, uint16_t* deq_up,
                                   int rows, int K, umv_stream_t stream);
/* M <= 64 only; a->wp = the MXFP4 image, a->w_scale = NULL; BIAS, RESIDUAL, SWIGLU, OUT_F32, row_idx and split-K partials as
 * umv_gemm_bf16; norm_w, th-row tiles and argmax_partial unsupported */
int umv_gemm_mxfp4w(const umv_gemm_args* a, umv_stream_t stream);
/* M > 64: the MFMA-tiled GEMM on the SAME MXFP4 image (a->wp), a->w_scale = NULL, K % 32 == 0 - an fp4 linear then needs no bf16 image
 * of W'.  BIAS, RESIDUAL, SWIGLU, OUT_F32, row_idx as umv_gemm_bf16; with k_splits > 1 (M <= 128) raw fp32 partials over umv_gemm_bf16's
 * K ranges (ceil(K/32 / k_splits) k-tiles of 32 per split, an empty range writes zeros).  One accumulator chain per output over k in
 * ascending 32-wide steps on v_mfma_f32_16x16x32_bf16:
 *   umv_gemm_mxfp4t(x, img)  ==  umv_gemm_bf16(x, pack(W'))   bit for bit, every M > 64, split-K partials included
 * norm_w, argmax_partial, th-row tiles and M <= 64 are UMV_ERR_UNSUPPORTED */
int umv_gemm_mxfp4t(const umv_gemm_args* a, umv_stream_t stream);

/* ------------------------------------------------------------------ exact 13-bit image of bf16 weights ("z13"; no reference
 * counterpart).  The decode GEMMs are HBM-bound and a bf16 weight's 8 exponent bits carry ~2.5 bits of entropy: this image keeps the
 * sign and the 7 mantissa bits as they are and codes the exponent field in 5 bits below a per-tile-pair base, WITHOUT LOSS:
 *   umv_gemm_z13w(x, pack_z13(W))  ==  umv_gemm_bf16(x, pack(W))   bit for bit, for every M <= 64, every K split, every epilogue
 * (finite x, the precondition of the full-line x staging of the weight-streaming kernels; umv_gemm_bf16 under its DEFAULT policy: its
 * tuning variables UMV_GEMM_SKINNY_MAX and UMV_GEMM_M64_TILED move 33..64-row calls between its weight-streaming kernel and an MFMA tile,
 * which sum in another order - the contract is not given for the rows they move).
 * Unit = a PAIR of 16-row n-tiles (2p, 2p + 1; a (gate, up) pair of a SwiGLU image) x 64 k.  NP = ceil(ceil(N/16) / 2), KT8 = K / 64
 * (K % 64 == 0, K <= 32768).  Image (umv_packed_weight_z13_bytes, 256-byte aligned):
 *   head   H[NP][16 B] at byte 0, per pair (one scalar load brings both to a workgroup):
 *            flags u64: bit b is set when rows of the pair hold, in k = [512 b, 512 b + 512), a weight that cannot be coded
 *                       (512 = the granule the decode kernel cuts K ranges by);
 *            base  u8:  the pair's largest exponent field BELOW 255 (0 when it has none); then 7 zero bytes;
 *   records R[p][k/64][3328 B] at byte roundup(16 NP, 256).  Lane = ((k%32)/8)*16 + n%16 holds the weights of the bf16 image's four
 *          fragments (tile 2p + tt, k half h = (k%64)/32, j = k%8), fragment number f = 2 tt + h:
 *            [0, 1024) / [1024, 2048): tile 2p / 2p + 1, 16 B per lane: byte 8 h + j = s << 7 | m7 (sign, mantissa);
 *            [2048, 3072): 16 B per lane, dword f: the low 4 bits of the code of weight j at bit 8 B(j) + 4 (j >> 2),
 *                          B(j) = 2 (j & 1) + ((j >> 1) & 1);
 *            [3072, 3328): 4 B per lane: the top bit of the code of (f, j) at bit 8 B(j) + 2 f + (j >> 2).
 *   code = base - exponent field, in 0..30 (31 is reserved and never written); bf16 bits = s << 15 | (base - code) << 7 | m7.  A field
 *   of 0 (zeros, subnormals) is a field like any other: codable when base <= 30, otherwise it flags - there is no zero code (it would
 *   cost the decode an instruction per two weights; trained weights and N(0, s^2) draws hold no zeros).
 *   Uncodable: field 255 (Inf / NaN) or more than 30 below the base.  Such a weight is written as code 0 and flags its block; rows at
 *   or beyond N (packed row order) and the missing tile of a ragged last pair never flag and do not count for the base.  The workgroups
 *   whose pairs and K range meet a set flag run the bf16 kernel on the bf16 image instead, so the bf16 image stays resident.
 * umv_pack_weight_z13 reads the PACKED bf16 image (umv_pack_weight_bf16 / _swiglu_bf16, the latter with N = 2 I, I % 16 == 0). */
size_t umv_packed_weight_z13_bytes(int N, int K);
int umv_pack_weight_z13(const uint16_t* packed16, uint8_t* z13, int N, int K, umv_stream_t stream);
/* M <= 64 only, 16-row images, K % 64 == 0; a->wp = the bf16 image (the fallback), z13 = its 13-bit image; BIAS, RESIDUAL, SWIGLU,
 * OUT_F32, row_idx, argmax_partial / sampling keys and split-K partials as umv_gemm_bf16; norm_w and th-row tiles are
 * UMV_ERR_UNSUPPORTED.  (33..64 rows of a SwiGLU / N >= 16384 GEMM, which umv_gemm_bf16 runs on an MFMA tile, run there.) */
int umv_gemm_z13w(const umv_gemm_args* a, const void* z13, umv_stream_t stream);
int umv_gemm_z13w_rows(const umv_gemm_args* a, const void* z13, const umv_row_sampling* rows, umv_stream_t stream);   /* see umv_gemm_bf16_rows */

/* W8A8 on the fp8 matrix instruction (v_mfma_scale_f32_16x16x128_f8f6f4) for the MFMA-bound GEMMs of the fp8 mode
 * (M > 64: prefill, flow passes).  Activations are quantised per ROW the way weights are per channel:
 *   sx[m] = smallest 2^e with 448 * 2^e >= max_k |x[m,k]|,  xq = rne_e4m3(x / sx)   (umv_quantize_act_fp8; rows may be
 *   gathered through row_idx; xq is [M, ldq] row-major, zero padded to ldq, a multiple of 128)
 *   out[m,n] = epilogue(sx[m] * sw[n] * sum_k xq[m,k] * wq[n,k])                    (umv_gemm_fp8a8w, fp32 accumulate)
 * Every product and both scales are exact, so the result equals a linear on the dequantised operands up to the order
 * of the fp32 sums - that is how oracle/fp8.py restates it.  The weight image for this instruction is a re-tiling of the
 * e4m3 image: P8M[n/16][k/128][(k%32)/16][lane = ((k%128)/32)*16 + n%16][k%16]. */
size_t umv_packed_weight_fp8_mfma_bytes(int N, int K);
int umv_repack_weight_fp8_mfma(const uint8_t* packed8, uint8_t* out, int N, int K, umv_stream_t stream);
/* deq (optional, row stride ldd): the dequantised rows as bf16 at their ORIGINAL positions (row_idx[m] when given) - the input
 * of the M <= 64 kernels, which take bf16 activations; xq may then be NULL */
int umv_quantize_act_fp8(const uint16_t* x, int64_t ldx, const int32_t* row_idx, uint8_t* xq, int64_t ldq, float* x_scale,
                         uint16_t* deq, int64_t ldd, int M, int K, umv_stream_t stream);
typedef struct {
    const uint8_t* xq;        /* [M, ldq] e4m3, rows 0..M-1 (already gathered) */
    int64_t ldq;
    const float* x_scale;     /* [M] */
    const uint8_t* wp;        /* umv_repack_weight_fp8_mfma image */
    const float* w_scale;     /* scales of umv_quantize_pack_weight_fp8 (image row order) */
    const uint16_t* bias;
    const uint16_t* residual;
    int64_t ldr;
    void* out;                /* bf16 [*, ldo] */
    int64_t ldo;
    const int32_t* row_idx;   /* optional [M]: residual / out rows (MoT routing); xq / x_scale are indexed by m */
    int M, N, K;
    int epilogue;             /* UMV_EPI_* except OUT_F32 */
} umv_gemm8_args;
int umv_gemm_fp8a8w(const umv_gemm8_args* a, umv_stream_t stream);

/* ------------------------------------------------------------------ norms / elementwise */
/* Qwen2RMSNorm (modeling_qwen2.py:89-94): out = w * bf16(x * rsqrt(mean(x^2)+eps)).
 * expert (optional, [T] int32): rows with expert[t]!=0 use w_gen (MoT *_moe_gen norms,
 * qwen2_navit.py:863-865,893-894,1166-1168).  row_idx optional gather/scatter. */
int umv_rmsnorm_bf16(const uint16_t* x, const uint16_t* w, const uint16_t* w_gen, const int32_t* expert,
                     uint16_t* out, int T, int H, float eps, umv_stream_t stream);
/* Consumer of a split-K decode GEMM (o_proj / down_proj, qwen2_navit.py:617-620, modeling_qwen2.py:235) fused with the
 * residual add (qwen2_navit.py:873-874,897-898) and the following Qwen2RMSNorm:
 *   seq[t,:] = bf16(bf16(sum_s partials[s*split_stride + t*ldp + :]) + seq[t,:])  (in place);  out = w * bf16(seq * rstd) */
int umv_residual_rmsnorm_bf16(const float* partials, int n_splits, int64_t split_stride, int64_t ldp, uint16_t* seq,
                              const uint16_t* w, uint16_t* out, int T, int H, float eps, umv_stream_t stream);
/* nn.LayerNorm with affine, bf16 in/out, fp32 statistics (siglip_navit.py:283,296,370) */
int umv_layernorm_bf16(const uint16_t* x, const uint16_t* w, const uint16_t* b, uint16_t* out, int T, int H,
                       float eps, umv_stream_t stream);
/* nn.Embedding gather (bagel.py:438,577,753,1092,1264): out[t,:] = table[ids[t],:]; optional
 * out_rows scatter (packed_sequence[packed_text_indexes] = ..., bagel.py:579) */
int umv_embed_gather_bf16(const uint16_t* table, const int64_t* ids, const int32_t* out_rows, uint16_t* out,
                          int T, int H, umv_stream_t stream);
/* out[rows[t],:] = bf16(a[t,:] + table[idx[t],:]) (+ optional second addend broadcast row `bcast`,
 * added first): connector + vit_pos_embed (bagel.py:590-595), vae2llm + t_emb + pos (bagel.py:1104-1109) */
int umv_add_rows_bf16(const uint16_t* a, const uint16_t* bcast, const uint16_t* table, const int64_t* idx,
                      const int32_t* out_rows, uint16_t* out, int T, int H, umv_stream_t stream);
/* greedy sampling (bagel.py:1301): argmax over bf16 logits, lowest index wins ties */
int umv_argmax_bf16(const uint16_t* logits, int64_t ld, int64_t* out_ids, int M, int V, umv_stream_t stream);
/* do_sample=True (bagel.py:1297-1299): token = multinomial(softmax(logits / temperature), 1), drawn as
 * argmax(p_i / q_i), q_i ~ Exp(1), from a counter-based generator keyed by (seed, *step, row, i); `step`
 * is an optional device counter so the call replays from a hipGraph.  Reproducible per seed; not torch's stream. */
int umv_sample_bf16(const uint16_t* logits, int64_t ld, int64_t* out_ids, int M, int V, float temperature, uint64_t seed,
                    const int64_t* step, umv_stream_t stream);
/* pixels [N, 3*p*p] fp32 -> bf16 [N, Kp] zero padded (cast that autocast applies before
 * the patch-embed linear, siglip_navit.py:190) */
int umv_cast_pad_f32_bf16(const float* x, int64_t ldx, uint16_t* out, int64_t ldo, int T, int K, int Kp,
                          umv_stream_t stream);
/* patchify (data/data_utils.py:43-50) + that cast on the device: transformed image [C, H, W] fp32 -> tokens
 * [(H/p)*(W/p), Kp] bf16, column (pp*p + qq)*C + c of token (ph, pw) = image[c][ph*p + pp][pw*p + qq], zero padded to Kp.
 * Replaces the host-side permute of prepare_vit_images (bagel.py:540-548) on the engine's own path. */
int umv_patchify_f32_bf16(const float* img, int C, int H, int W, int p, uint16_t* out, int64_t ldo, int Kp, umv_stream_t stream);

/* ------------------------------------------------------------------ attention
 * KV slab layout (replaces NaiveCache's re-merged [sum K, kvh, hd] tensors,
 * qwen2_navit.py:207-221,585-600): per layer
 *   K  [seg][kv_head][cap][hd]   V^T [seg][kv_head][hd][cap]    (cap % 32 == 0)
 * V is kept transposed so that P.V consumes 16-byte key-contiguous MFMA fragments. */

/* per-head q/k RMSNorm + RoPE + cast + in-place KV append (qwen2_navit.py:544-545,568-583,
 * 585-600,622-624; modeling_qwen2.py:196-220).  qkv [T, (nq+2*nkv)*hd] from the fused QKV GEMM.
 * tok_seg/tok_slot/tok_pos: [T] int32 slab segment, slot in slab, rope position.
 * expert[t]!=0 -> the *_moe_gen norm weights; fp32_chain!=0 -> the whole call follows the
 * "gen" rounding chain (norm + rope in fp32, one final cast), as mode=="gen" does for text
 * and latent tokens alike.
 * cos/sin tables [max_pos, hd] bf16 as Qwen2RotaryEmbedding returns them (modeling_qwen2.py:184). */
typedef struct {
    const uint16_t* qkv;
    uint16_t* q_out; /* [T, nq, hd] bf16 */
    uint16_t* k_slab;
    uint16_t* vt_slab;
    int64_t k_seg_stride, k_head_stride, v_seg_stride, v_head_stride, v_d_stride;
    const int32_t *tok_seg, *tok_slot, *tok_pos, *expert;
    const uint16_t *q_norm_w, *k_norm_w, *q_norm_w_gen, *k_norm_w_gen; /* NULL norm -> no norm/rope (ViT) */
    const uint16_t *cos_tab, *sin_tab;
    int T, nq, nkv, hd;
    float eps;
    int fp32_chain;
    /* optional: take the fused QKV row from a split-K GEMM (umv_gemm_args.k_splits) instead of `qkv`:
     * x = bf16(sum_s qkv_partials[s*split_stride + t*(nq+2nkv)*hd + col] + qkv_bias[col]), splits in order 0..S-1 */
    const float* qkv_partials;
    int n_splits;
    int64_t split_stride;
    const uint16_t* qkv_bias;
    /* Paged KV (optional): page_table as in umv_attn_args - token t goes to page page_table[tok_seg[t] * page_table_stride + tok_slot[t] / 256],
     * in-page slot tok_slot[t] % 256; k_slab / vt_slab are the pools, *_seg_stride the page strides, v_d_stride = 256 */
    const int32_t* page_table;
    int page_table_stride;
} umv_qkv_post_args;
int umv_qkv_post(const umv_qkv_post_args* a, umv_stream_t stream);

/* flash_attn_varlen_func(q,k,v,cu_seqlens_q,cu_seqlens_k,max_q,max_k,causal) as used at
 * qwen2_navit.py:605-614 and siglip_navit.py:232-241: softmax scale 1/sqrt(hd), fp32
 * softmax, causal = bottom-right aligned.  Keys come from the slabs; kv_len[s] counts
 * the keys visible to segment s (including this call's new tokens).  nsplit>1 splits
 * the key range (decode) and needs workspace of umv_attn_workspace_bytes(). */
typedef struct {
    const uint16_t* q; /* [T, nq, hd] */
    uint16_t* out;     /* [T, nq, hd] */
    const int32_t* cu_q;
    const int32_t* kv_len;
    const uint16_t* k_slab;
    const uint16_t* vt_slab;
    int64_t k_seg_stride, k_head_stride, v_seg_stride, v_head_stride, v_d_stride;
    int nseg, nq, nkv, hd, causal;
    int max_q;  /* upper bound of query rows per segment (grid sizing) */
    int max_kv; /* upper bound of kv_len (grid sizing for nsplit) */
    int nsplit;
    void* workspace;
    /* Optional in-place operands (0 = the defaults above).  q_row_stride: elements between consecutive query rows (default
     * nq*hd; the q columns of a fused [T, (nq+2nkv)*hd] QKV buffer are read where the GEMM left them).  k_key_stride > 0: K is
     * NOT a slab but a packed [T, ...] buffer like q - key p of segment s is row cu_q[s] + p, k_slab points at its first K
     * column, k_head_stride is the head pitch inside a row, k_seg_stride is ignored (self-attention without a cache: the
     * SigLIP tower, siglip_navit.py:232-241).  V^T always comes from vt_slab. */
    int64_t q_row_stride, k_key_stride;
    /* Optional, for tests and A/B runs (0 / NULL in production).  variant: 0 = the library's own shape -> kernel policy; with
     * UMV_ATTN_VARIANT_FORCE set, the other UMV_ATTN_VARIANT_* bits pick the nsplit = 1 kernel for THIS call (a per-call value: the
     * library keeps no mutable state).  stats: two device counters the lazy-softmax kernels add to - [0] the (wave, q-tile, 32-key block)
     * events in which the softmax reference moved on a NON-EMPTY accumulator (O and l rescaled by alpha), [1] those in which a row's
     * reference was set for the first time. */
    int variant;
    uint32_t* stats;
    /* Paged KV (optional): page_table [nseg][page_table_stride] int32 - entry p of segment s is the pool page holding its keys
     * p*256 .. p*256+255.  k_slab / vt_slab are then page POOLS, K [page][kv_head][256][hd], V^T [page][kv_head][hd][256]: k_seg_stride /
     * v_seg_stride = elements per page, v_d_stride = 256; a pool is at most 2 GiB (32-bit offsets of the LDS-shared prefill kernels, whose
     * PAGED instantiations give the slab call's bits; hd 72 / exact-maximum variants of a paged call run on the per-wave kernel).  wave_split = 2 / 4 (decode, max_q rows in one q-tile, hd 128): the waves of a workgroup split its key
     * range and merge in LDS, so the same parallelism needs nsplit / wave_split partials for the combine. */
    const int32_t* page_table;
    int page_table_stride;
    int wave_split;
} umv_attn_args;
#define UMV_KV_PAGE 256
#define UMV_KV_PAGE_LOG2 8
enum {
    UMV_ATTN_VARIANT_FORCE = 1,        /* the bits below replace the process policy (and its UMV_ATTN_* environment knobs) */
    UMV_ATTN_VARIANT_STREAM = 2,       /* the per-wave streaming kernel (attn_kernel) even where the LDS-shared kernels would run */
    UMV_ATTN_VARIANT_TQ1 = 4,          /* LDS-shared kernel, one q-tile per wave */
    UMV_ATTN_VARIANT_TQ2 = 8,          /* ... two q-tiles per wave (neither bit: by grid size) */
    UMV_ATTN_VARIANT_EXACT = 16,       /* exact running maximum (the bits of attn_kernel) instead of the lazy softmax reference */
    UMV_ATTN_VARIANT_WHOLE_TOKENS = 32 /* q-tiles of whole tokens instead of densely packed (token, head) pairs */
};                                     /* (other bits are ignored) */
size_t umv_attn_workspace_bytes(int nseg, int nq, int hd, int max_q, int nsplit);
int umv_attn_varlen(const umv_attn_args* a, umv_stream_t stream);
/* Host-only query: which kernel an nsplit = 1 call goes to: 0 = per-wave streaming kernel, 1 / 2 = the LDS-shared
 * prefill kernel with 1 / 2 query tiles per wave (2 needs >= 512 workgroups). */
int umv_attn_prefill_tq(int nseg, int nq, int nkv, int hd, int max_q);


/* decode bookkeeping kept on device so a whole step replays from a hipGraph:
 * slot[b]+=1, pos[b]+=1, kv_len[b]+=1 (the .tolist() bookkeeping of bagel.py:1266-1275,1303-1310) */
int umv_decode_advance(int32_t* tok_slot, int32_t* tok_pos, int32_t* kv_len, int B, umv_stream_t stream);
/* The same plus the token log of the loop, one launch at the end of a step: with s = step_idx[0],
 * pred_ids[s][b] = ids[b] (the curr_tokens appended at bagel.py:1311-1312), in_ids[s+1][b] = ids[b] (what the next step is fed;
 * in_ids[0] holds the start tokens, bagel.py:1263), counters += 1, step_idx[0] = s + 1.  in_ids / pred_ids are [max_len][B]. */
int umv_decode_step_end(int32_t* tok_slot, int32_t* tok_pos, int32_t* kv_len, const int64_t* ids, int64_t* in_ids,
                        int64_t* pred_ids, int64_t* step_idx, int B, int max_len, umv_stream_t stream);
/* umv_decode_step_end with the greedy pick folded in: ids[b] = column of the maximum key of argmax_partial[b][0..n_tiles)
 * (written by umv_gemm_bf16 / umv_gemm_fp8w with argmax_partial set), then the bookkeeping above.  `ids` is an OUTPUT here
 * (the token the next step embeds).  One workgroup per sample, and one step counter PER SAMPLE: step_idx has B entries (all
 * equal; the caller zeroes them), workgroup b reads and advances step_idx[b] - no word is shared between workgroups. */
int umv_decode_step_end_argmax(int32_t* tok_slot, int32_t* tok_pos, int32_t* kv_len, const uint64_t* argmax_partial, int n_tiles,
                               int64_t* ids, int64_t* in_ids, int64_t* pred_ids, int64_t* step_idx, int B,
                               int max_len, umv_stream_t stream);

/* ------------------------------------------------------------------ token log-probabilities
 * For row b of a decode step let y[n] be the value the token pick orders, without noise: greedy, y[n] = float(bf16 logit[b][n]), exactly
 * the value stored to `out`; sampling at temperature T > 0, y[n] = bf16_round(logit[b][n] / T) (bagel.py:1297-1299: logits / temperature
 * is a bf16 tensor).  Then logprob(b, id) = y[id] - logsumexp_n y[n] in fp32: a -inf column contributes 0, a row with a NaN logit
 * gives NaN.  Inputs are bf16, so y[id] and the maximum are exact; measured against fp64 the value is within 1e-4 for |logprob| <= 200.
 *
 * umv_decode_step_end_logprob = umv_decode_step_end_argmax (same arguments, same bookkeeping, one workgroup and one step counter per
 * sample) that also merges the tiles' (m_t, s_t) of lse_partial [B][n_tiles][2]: M = max m_t, S = sum s_t * exp(m_t - M), in a fixed
 * order (thread-strided, the wave tree, waves 0..3), reads y[id] back from the logits the GEMM stored (`logits`, row stride ldo
 * elements, V columns; temperature as given to the GEMM, 0 = greedy) and writes logprob[s * B + b] (fp32 [max_len][B]).
 * forced_ids (optional, [max_len][B]): where forced_ids[s][b] >= 0 that token becomes ids[b] and in_ids[s + 1][b] and the
 * log-probability is its own, while pred_ids[s][b] still records the model's pick; a negative entry leaves the sample free-running
 * at that step.  A forced token >= V is never fed: the step free-runs and its log-probability is NaN. */
int umv_decode_step_end_logprob(int32_t* tok_slot, int32_t* tok_pos, int32_t* kv_len, const uint64_t* argmax_partial,
                                const float* lse_partial, int n_tiles, int64_t* ids, int64_t* in_ids, int64_t* pred_ids,
                                int64_t* step_idx, const uint16_t* logits, int64_t ldo, int V, float temperature,
                                const int64_t* forced_ids, float* logprob, int B, int max_len, umv_stream_t stream);
/* The stand-alone form over bf16 logits [M][V] (row stride ld elements): out[m] = logprob(m, ids[m]) by the definition above, one
 * workgroup per row.  temperature = 0: greedy (T = 1 without the rounding step).  An id outside [0, V) gives NaN. */
int umv_token_logprob_bf16(const uint16_t* logits, int64_t ld, const int64_t* ids, float* out, int M, int V, float temperature,
                           umv_stream_t stream);
/* Token log-probabilities of given rows, no logits stored (the prefill-time scorer: every row of a teacher-forced pass against the
 * token that follows it).  The greedy form of the definition above, for ANY number of rows: for row m with hidden state x[m] and
 * target ids[m],
 *   y[n]    = float(bf16(lm_head(x[m])[n] (+ bias[n]))), exactly the value umv_gemm_bf16 would store to `out`;
 *   logprob = y[ids[m]] - logsumexp_n y[n] in fp32, through the per-16-column-tile (m_t, s_t) of lse_partial above, in its order, merged
 *             in umv_decode_step_end_logprob's order.  A -inf column adds 0, a NaN logit gives NaN, an id outside [0, V) gives NaN.
 *
 * umv_lm_head_stats_bf16: the lm_head GEMM on an MFMA tile (every M >= 1; one accumulator chain per output over k in ascending 32-wide
 * steps, as umv_gemm_bf16 on any of its tiles, so y is the bf16 value that call stores) whose epilogue writes
 *   lse_partial [M][ceil(N/16)][2] fp32: (m_t, s_t) of every tile of every row - each entry of rows < M is written;
 *   target_y [M] fp32: y[ids[m]], where ids[m] (int64 [M], device memory) lies in [0, N); otherwise the entry is left alone
 * and NO logits: a->out may be NULL and is ignored.  The struct is umv_gemm_args unchanged; of its fields the call takes x, ldx, wp (the
 * umv_pack_weight_bf16 image), M, N, K and bias with UMV_EPI_BIAS.  UMV_ERR_ARG: a NULL x / wp / ids / lse_partial / target_y, a bad
 * shape, a->lse_partial set.  UMV_ERR_UNSUPPORTED: row_idx, residual, norm_w, k_splits > 1, tile_rows other than 0 / 16, any epilogue
 * flag but UMV_EPI_BIAS, argmax_partial, sample_temperature != 0.
 *
 * umv_token_logprob_from_stats: one workgroup per row merges lse_partial [M][n_tiles][2] as umv_decode_step_end_logprob does and
 * writes out[m] = (target_y[m] - ref) - logf(S), NaN for ids[m] outside [0, V) - given the same statistics and y, that entry's bits.
 * UMV_ERR_ARG: a NULL pointer, V that is not the column count behind n_tiles. */
int umv_lm_head_stats_bf16(const umv_gemm_args* a, const int64_t* ids, float* lse_partial, float* target_y, umv_stream_t stream);
int umv_token_logprob_from_stats(const float* lse_partial, int n_tiles, const float* target_y, const int64_t* ids, int V, float* out, int M,
                                 umv_stream_t stream);

/* ------------------------------------------------------------------ truncated sampling: top-k, top-p (nucleus), min-p
 * For one row, y[n] = bf16_round(logit[n] / T), T > 0 - the value the sampling keys and the log-probabilities above use.  A CLASS is the
 * set of columns that share one value of y (-0 == +0; at most 65 536 classes).  Every filter keeps or drops whole classes, so a tie is
 * never split, and the kept set is always "every column whose y is at or above a cutoff value":
 *   top_k (int, 0 = off): every class at or above the k-th largest value of the row - ties with the k-th value are kept (the rule of
 *     HF's TopKLogitsWarper), so n_kept >= min(k, V);
 *   top_p (float in (0, 1], 1 = off): applies to what top_k kept, whose mass is Z_k: the smallest set of highest classes whose mass
 *     reaches top_p * Z_k.  The mass of a class is count * expf(y - M), M the row maximum (the top class weighs count * 1 whatever
 *     its value), accumulated over the classes in descending order in fp64;
 *   min_p (float in [0, 1), 0 = off): the classes with y - M >= logf(min_p).
 * The cutoff is the highest of the three, so the top class is always kept.  The token is the argmax over the kept columns of
 * bf16_round(logit / T) + Gumbel noise, lowest column on equal keys - the noise of the lm_head sampling epilogue (argmax_partial with
 * sample_temperature > 0), keyed by (seed, step, row, column), so where the untruncated pick is itself kept it IS the truncated pick.
 * Consequences: a NaN logit ranks highest and wins, as in the untruncated sampler (the NaN columns are the kept set, cut_y is NaN);
 * a row of -inf only is one class and behaves as the untruncated sampler does; top_k = 1 picks from the top class - greedy unless the
 * maximum is tied; token log-probabilities keep their definition, that of the UNTRUNCATED softmax(y).  With all three filters off
 * there is nothing to truncate: both entries return UMV_ERR_ARG (the untruncated sampler is umv_sample_bf16 / the sampling epilogue
 * with umv_decode_step_end_argmax or _logprob), as they do for top_k < 0, top_p outside (0, 1], min_p outside [0, 1), T <= 0.
 * The cutoff is found from integer class counts and fixed-order fp64 sums: a row's result does not depend on the batch it sits in.
 *
 * umv_sample_truncated_bf16: the stand-alone form over bf16 logits [M][V] (row stride ld elements), one workgroup per row.  step: device
 * pointer to the step counter (NULL = 0), as umv_sample_bf16's.  cut_y (fp32 [M], may be NULL) receives the cutoff value, n_kept
 * (int32 [M], may be NULL) the number of kept columns. */
int umv_sample_truncated_bf16(const uint16_t* logits, int64_t ld, int64_t* out_ids, int M, int V, float temperature, uint64_t seed,
                              const int64_t* step, int top_k, float top_p, float min_p, float* cut_y, int32_t* n_kept,
                              umv_stream_t stream);
/* The step end of a truncated sampling step: umv_decode_step_end_logprob's arguments, bookkeeping and per-sample step counters, after
 * an lm_head GEMM that sampled with (temperature, seed, step_idx) into argmax_partial.  Per sample it finds the cutoff from the stored
 * logits, keeps the untruncated pick of argmax_partial if y[pick] >= cutoff, and takes the Gumbel maximum over the kept columns with
 * regenerated noise otherwise.  logprob and lse_partial may be NULL together (no log-probabilities).  cut_y (fp32 [max_len][B]) and
 * n_kept (int32 [max_len][B]) receive row s like logprob; either may be NULL. */
int umv_decode_step_end_truncated(int32_t* tok_slot, int32_t* tok_pos, int32_t* kv_len, const uint64_t* argmax_partial,
                                  const float* lse_partial, int n_tiles, int64_t* ids, int64_t* in_ids, int64_t* pred_ids,
                                  int64_t* step_idx, const uint16_t* logits, int64_t ldo, int V, float temperature,
                                  const int64_t* forced_ids, float* logprob, int B, int max_len, uint64_t seed, int top_k, float top_p,
                                  float min_p, float* cut_y, int32_t* n_kept, umv_stream_t stream);

/* ------------------------------------------------------------------ logit penalties and bias
 * Repetition, presence and frequency penalties and a static logit bias, applied to the stored bf16 logits of a decode step BEFORE
 * anything picks from them.  For row b let l[n] = float(stored bf16 logit), c[n] the number of times column n was generated so far in
 * this request (the tokens fed at steps 1..s - the model's picks, or the forced tokens where they were fed; the start token is not
 * counted), P an optional set of context (prompt) columns, bias[n] an optional fp32 bias (0 where absent, -inf bans a column) and
 * seen(n) = c[n] > 0 or n in P.  The adjusted logit is formed in fp32, one rounding per operation, nothing contracted to an FMA:
 *     a = l[n]
 *     if seen(n) and r != 1:  a = (a < 0) ? a * r : a / r             repetition_penalty r > 0 (the HF / CTRL rule; includes P)
 *     if c[n] > 0:            a = a - (presence + frequency * float(c[n]))   product, sum, difference (the OpenAI rule; generated only)
 *     if bias[n] != 0:        a = a + bias[n]
 *     l'[n] = bf16_round_nearest_even(a)
 * NaN stays NaN and -inf stays -inf (bias = +inf on a -inf logit is the NaN the arithmetic gives); a column that is neither seen nor
 * biased, and every column while r = 1, presence = frequency = 0 and bias = 0, keeps its bits.  l' REPLACES l in memory, and everything
 * downstream is defined on l' in the words used above: the greedy pick, y = bf16(l' / T) and its Gumbel key, the token
 * log-probabilities - those of the ADJUSTED, untruncated softmax - and the truncation classes.  So penalties come before temperature and
 * before truncation (the order of HF's logits processors).  A row's result depends only on its own logits, history, context and bias.
 *
 * umv_logit_penalty_bf16: one workgroup per row, between the lm_head GEMM and whatever picks.  Per row, in this order:
 *   record   list_len[b] < 0 marks a FRESH slot: the word becomes n_static and nothing is counted (ids[b] is the start token).
 *            Otherwise c[ids[b]] += 1 and, if that column is not listed yet and list_len[b] < cap, it is appended to the row's visit
 *            list.  Nothing is ever written at or beyond cap (a column that found no room is counted but not penalised).  An id
 *            outside [0, V) is ignored.
 *   patch    every list entry is one column, handled by one thread: l[n] -> l'[n].  The list is distinct by construction, so no column
 *            is patched twice.
 *   tiles    with argmax_partial: for every list entry the whole 16-column tile is recomputed from the patched row and
 *            argmax_partial[b][tile] - and lse_partial[b][tile] when given - stored, with the bits the lm_head epilogue of
 *            umv_gemm_bf16 leaves for those logits: greedy keys when temperature = 0, the sampling keys of (temperature, seed, *step)
 *            otherwise.  argmax_partial = NULL: record and patch only (the unfused step, where umv_argmax_bf16 / umv_sample_bf16 read
 *            the logits afterwards).
 * Memory.  count [M][V] int32: bits 0..29 c[n] (saturating), bit 30 (UMV_PENALTY_CONTEXT) n is in P, bit 31 (UMV_PENALTY_LISTED) n is
 * in the row's list; the caller zeroes a row and sets the two flags of its static columns.  list [M][cap] int32: entries 0..n_static-1
 * are the STATIC ones the caller seeds - the context and bias columns, distinct, -1 = unused - and bias [M][n_static] fp32 (may be NULL)
 * runs parallel to them; the generated columns follow from n_static on.  list_len [M] int32: the caller writes -1 to start a request.
 * UMV_ERR_ARG: repetition_penalty <= 0 or not finite, presence / frequency not finite, temperature < 0, lse_partial without
 * argmax_partial, cap < n_static, n_tiles that is not ceil(V / 16) with argmax_partial. */
#define UMV_PENALTY_COUNT_MASK 0x3FFFFFFFu
#define UMV_PENALTY_CONTEXT 0x40000000u
#define UMV_PENALTY_LISTED 0x80000000u
typedef struct {
    uint16_t* logits;          /* [M][V] bf16, row stride ld elements; patched in place */
    int64_t ld;
    const int64_t* ids;        /* [M]: the token each row is fed at this step */
    int32_t* count;            /* [M][V] */
    int32_t* list;             /* [M][cap] */
    int32_t* list_len;         /* [M] */
    const float* bias;         /* [M][n_static] or NULL */
    int M, V, cap, n_static;
    float repetition_penalty, presence_penalty, frequency_penalty;
    float temperature;         /* as given to the lm_head GEMM: 0 = greedy keys and y = l' */
    uint64_t* argmax_partial;  /* optional [M][n_tiles] */
    float* lse_partial;        /* optional [M][n_tiles][2], only with argmax_partial */
    int n_tiles;
    uint64_t seed;             /* sample_seed / sample_step of the lm_head call (temperature > 0) */
    const int64_t* step;
    const umv_row_sampling* rows; /* optional [M] ("per-row sampling parameters"): r / presence / frequency of row b are rows[b]'s, and the
                                  tiles are recomputed with rows[b]'s temperature and (seed, draw, stream).  The scalar fields must then
                                  be neutral - repetition_penalty 1, presence / frequency 0, temperature 0 - UMV_ERR_ARG otherwise.
                                  Read only. */
} umv_logit_penalty_args;
int umv_logit_penalty_bf16(const umv_logit_penalty_args* a, umv_stream_t stream);

/* ------------------------------------------------------------------ per-row sampling parameters
 * One captured decode step can serve rows with different samplers: a table of umv_row_sampling (above), one entry per row, replaces
 * the scalar temperature / seed / step / filters / penalties of the entries above.  EVERY per-row definition is the scalar definition
 * with the row's own values: the sampling key of row m, column n is that of umv_gemm_args.sample_temperature with
 *   (sample_seed, *sample_step, m)  :=  (rows[m].seed, rows[m].draw, rows[m].stream),
 * i.e. row key = splitmix64(seed ^ draw * 0xD1B54A32D192ED03 ^ (uint64_t)stream << 32); y, the log-probabilities, the truncation
 * classes and the penalties are those of the sections above with rows[m].temperature, top_k / top_p / min_p and the three penalty
 * values.  So a table whose rows all hold the values of a scalar call, with stream = m and draw = *sample_step, leaves the bits of that
 * scalar call; and a request's draws depend only on its own (seed, stream, draw), not on the row it sits in.
 * A row with temperature > 0 samples; any other temperature (0, negative, NaN) marks a GREEDY row: greedy keys, y = the logit, and
 * the row's filters are ignored.  Greedy and sampled rows may share a call, a workgroup and a 16-row fragment.
 * The GEMMs and the penalty kernel only read the table.
 *
 * umv_decode_step_end_rows: the step end of such a step - umv_decode_step_end_truncated's arguments without the scalar temperature /
 * seed / top_k / top_p / min_p, plus the table, one workgroup per sample.  Per row:
 *   temperature > 0 and a filter on (top_k > 0, top_p < 1 or min_p > 0): umv_decode_step_end_truncated's pick with the row's values;
 *   otherwise: the maximum of the row's keys (umv_decode_step_end_argmax / _logprob); cut_y = -inf, n_kept = V.
 * logprob and lse_partial may be NULL together; forced_ids, cut_y and n_kept as in umv_decode_step_end_truncated.  Last, thread 0 of
 * the row's workgroup stores rows[b].draw + 1 to rows[b].draw - the only word of the table anything writes.  UMV_ERR_ARG: a NULL or
 * misaligned table, logprob without lse_partial (or the reverse), V that is not the column count behind n_tiles. */
int umv_decode_step_end_rows(int32_t* tok_slot, int32_t* tok_pos, int32_t* kv_len, const uint64_t* argmax_partial,
                             const float* lse_partial, int n_tiles, int64_t* ids, int64_t* in_ids, int64_t* pred_ids,
                             int64_t* step_idx, const uint16_t* logits, int64_t ldo, int V, const int64_t* forced_ids, float* logprob,
                             int B, int max_len, umv_row_sampling* rows, float* cut_y, int32_t* n_kept, umv_stream_t stream);

/* ------------------------------------------------------------------ top-n alternative tokens and token ranks
 * For row b of a decode step take y[c] exactly as the token log-probabilities define it: greedy (temperature 0) y[c] = float(bf16
 * logit), temperature T > 0 y[c] = bf16_round(logit / T) - with a per-row table the row's own temperature - and -0 == +0.  The logits
 * are the stored ones, so after umv_logit_penalty_bf16 the adjusted ones; the alternatives are those of the UNTRUNCATED softmax, like
 * the log-probabilities.  Order the columns by (y descending, column ascending): argmax_key's order applied to y without noise.
 *   top_ids[j], j = 0..n-1: the j-th column in that order.
 *   top_logprobs[j] = (y[top_ids[j]] - ref) - logf(S), with (ref, S) the row's merged statistics, merged in exactly the order of the
 *     step end that ended the step - so wherever the fed token is one of the n, its entry equals that step end's logprob bit for bit.
 *   rank = 1 + the number of columns before the FED token in that order, int32, 1-based.  The fed token is the one the step end left
 *     for the next step (ids[b] = in_ids[s + 1][b]): the pick, or the forced token where one was fed.  0 where the forced token was
 *     outside the vocabulary (forced_ids[s][b] >= V) or the stand-alone id is outside [0, V).
 * Ties are split by column, never by the logit: at T > 0 two different logits can share one y (3.015625 and 3.03125 both give 2.015625
 * at T = 1.5), and then the lower column comes first even if its logit is the smaller one.  -inf columns are ordinary: last in the
 * order, log-probability -inf.  A row whose merged S is NaN (a NaN logit) gives NaN in every top_logprobs entry, -1 in every top_ids
 * entry and rank 0.  All comparisons are integer or exact bf16: a row's ids and ranks never depend on the batch it sits in, and neither
 * do its log-probabilities under the condition the token log-probabilities have.  1 <= n <= UMV_TOP_LOGPROBS_MAX and n <= V,
 * UMV_ERR_ARG otherwise, as for a NULL output.
 *
 * umv_decode_top_logprobs: one launch AFTER the step end of a step (umv_decode_step_end_logprob, _truncated or _rows), one workgroup
 * per sample, no word shared between workgroups.  The step just ended is s = step_idx[b] - 1; row s of top_ids (int32
 * [max_len][B][n]), top_logprobs (fp32 [max_len][B][n]) and rank (int32 [max_len][B]) is written; s outside [0, max_len) writes
 * nothing.  logits / ldo / V / lse_partial / n_tiles / forced_ids: what the step end got.  ids [B]: the tokens the step end left for
 * the next step.  temperature: the scalar one (0 = greedy), ignored where rows (optional, the table of umv_decode_step_end_rows) is
 * given - then row b's own temperature applies.  merge_order names the step end whose order the statistics are merged in:
 * UMV_TOP_AFTER_LOGPROB or UMV_TOP_AFTER_TRUNCATED; with rows it is ignored and the row's own is taken (a sampled row with a filter on:
 * the truncated one).
 *
 * umv_top_logprobs_bf16: the stand-alone form over bf16 logits [M][V] (row stride ld elements) with ids [M], whose rank is wanted; the
 * statistics come from the logits as umv_token_logprob_bf16 takes them (its bits), outputs are [M][n] / [M][n] / [M]. */
#define UMV_TOP_LOGPROBS_MAX 20
#define UMV_TOP_AFTER_LOGPROB 0
#define UMV_TOP_AFTER_TRUNCATED 1
int umv_decode_top_logprobs(const uint16_t* logits, int64_t ldo, int V, const float* lse_partial, int n_tiles, float temperature,
                            const umv_row_sampling* rows, int merge_order, const int64_t* ids, const int64_t* step_idx,
                            const int64_t* forced_ids, int B, int max_len, int n, int32_t* top_ids, float* top_logprobs, int32_t* rank,
                            umv_stream_t stream);
int umv_top_logprobs_bf16(const uint16_t* logits, int64_t ld, const int64_t* ids, int M, int V, float temperature, int n,
                          int32_t* top_ids, float* top_logprobs, int32_t* rank, umv_stream_t stream);

/* ------------------------------------------------------------------ token automata: constrained decoding
 * Which tokens a row may be fed next, as a function of what it was fed so far: a deterministic automaton over token ids in CSR form,
 * read-only device memory.  State s owns the edges row_ptr[s] .. row_ptr[s + 1] - 1; edge e carries the token edge_token[e] and the
 * state edge_next[e] the row is in after that token.  Within a state the tokens are strictly ascending (sorted, distinct).  Each row
 * carries one int32 state word in device memory (state [M]).  A word that is negative or >= n_states marks a FREE row: unconstrained.
 * UMV_CONSTRAINT_FREE as an edge_next releases the row; UMV_CONSTRAINT_LEFT is what the word becomes when the row is fed a token its
 * state has no edge for (a forced token, say) - unconstrained from then on, and told apart from a released row.
 *
 * umv_logit_constrain_bf16: between the lm_head GEMM and whatever picks, after umv_logit_penalty_bf16 when that runs; grid (chunk of
 * UMV_CONSTRAIN_CHUNK columns, row).  For row b with s = state[b]:
 *   free     s < 0 or s >= n_states: no byte of the row's logits, keys or statistics is written.
 *   masked   otherwise let A be the tokens of s's edges that lie in [0, V) (an edge token >= V is ignored).  Every column outside A
 *            becomes bf16 -inf (0xFF80) - a NaN outside A too -, every column in A keeps its bits, NaN included.  The masked row
 *            REPLACES the logits in memory, as the penalties' l' does, and everything downstream is defined on it in the words used
 *            above: the greedy pick, y = bf16(l / T) and its Gumbel key, the truncation classes, the token log-probabilities - now
 *            those of the softmax renormalised over A -, the top-n alternatives.
 *   tiles    with argmax_partial (and lse_partial when given) EVERY tile of a masked row holds the bits the lm_head epilogue of
 *            umv_gemm_bf16 leaves for the masked logits: greedy keys when temperature = 0, the sampling keys of (temperature, seed,
 *            *step) otherwise - with rows, of rows[b]'s temperature and (seed, draw, stream); the statistics in epi_lse_tile's
 *            order.  A tile without an allowed column holds the key of -inf at its lowest column and (-inf, 0).  argmax_partial =
 *            NULL: the logits only (the unfused step).
 *   empty A  legal: the row of -inf only, which behaves as such a row does everywhere above.
 * The kernel only reads state.  UMV_ERR_ARG: what umv_logit_penalty_bf16 rejects of the fields the two share (temperature < 0 or
 * not finite, lse_partial without argmax_partial, n_tiles that is not ceil(V / 16) with argmax_partial, rows with a scalar
 * temperature other than 0, a misaligned table), a NULL state, row_ptr or - with n_edges > 0 - edge array, n_states <= 0,
 * n_edges < 0.  The automaton's CONTENTS are the caller's: nothing is validated on the device; what the kernels guarantee for a
 * malformed table is only that they read nothing outside its n_edges edges and write nothing outside the row.
 *
 * umv_constraint_advance: after the step end (and after umv_decode_top_logprobs), one thread per row and a binary search.  ids [M]:
 * the token the step end left to be fed next, picked or forced.  A row whose word is negative or >= n_states keeps it; otherwise
 * state[b] becomes the edge_next of state[b]'s edge for ids[b], or UMV_CONSTRAINT_LEFT when there is none.  state[b] is the only word
 * written, and this entry the only writer: a constrained step is lm_head, [penalty], constrain, step end, [top-logprobs], advance -
 * one graph, no host round trip, no word shared between workgroups. */
#define UMV_CONSTRAINT_FREE (-1)
#define UMV_CONSTRAINT_LEFT (-2)
#define UMV_CONSTRAIN_CHUNK 4096
typedef struct {
    const int32_t* row_ptr;     /* [n_states + 1], ascending, row_ptr[0] = 0 */
    const int32_t* edge_token;  /* [n_edges]; within a state strictly ascending */
    const int32_t* edge_next;   /* [n_edges]; a state, or UMV_CONSTRAINT_FREE */
    int n_states, n_edges;
} umv_token_automaton;
typedef struct {
    uint16_t* logits;          /* [M][V] bf16, row stride ld elements; masked in place */
    int64_t ld;
    int M, V;
    umv_token_automaton automaton;
    const int32_t* state;      /* [M] */
    float temperature;         /* as given to the lm_head GEMM: 0 = greedy keys and y = l */
    uint64_t* argmax_partial;  /* optional [M][n_tiles] */
    float* lse_partial;        /* optional [M][n_tiles][2], only with argmax_partial */
    int n_tiles;
    uint64_t seed;             /* sample_seed / sample_step of the lm_head call (temperature > 0) */
    const int64_t* step;
    const umv_row_sampling* rows; /* optional [M]: row b's temperature and (seed, draw, stream); the scalar temperature must be 0 */
} umv_logit_constrain_args;
int umv_logit_constrain_bf16(const umv_logit_constrain_args* a, umv_stream_t stream);
int umv_constraint_advance(const umv_token_automaton* automaton, int32_t* state, const int64_t* ids, int M, umv_stream_t stream);

/* ------------------------------------------------------------------ no-repeat n-grams
 * no_repeat_ngram_size: a row may not emit a token that would complete an n-gram its history already holds.  Row b owns an ordered
 * history h[0..L): hist [M][hist_ld] int32 with its length in hist_len[b].  The caller seeds it with an optional context (the prompt's
 * tokens; negative entries are separators); the kernel appends the token the step is fed, ids[b] - the start token and any forced
 * token included (an id outside [0, 2^31) is recorded as -1).  Let L be the length after the append and n the row's size: row_n[b]
 * where that optional int32 [M] array is given, else the scalar n.  A row with n outside 1..UMV_NGRAM_MAX is recorded but not banned.
 *   banned set  Ban = { h[i + n - 1] : 0 <= i <= L - n, h[i .. i + n - 1) == h[L - n + 1 .. L) element for element }.  All compared
 *               entries must lie in [0, V): a separator or an out-of-range id never matches.  A follower outside [0, V) is not banned.
 *               n = 1 bans every history token; L < n bans nothing; the candidate i = L - n overlaps the suffix and counts (history
 *               a a, n = 2: a is banned).  This is HF's NoRepeatNGramLogitsProcessor applied to the sequence h.
 *   column      a banned column becomes bf16 -inf (0xFF80), also where it held NaN; a column already -inf stays -inf; every other
 *               column keeps its bits.  The banned row REPLACES the logits in memory, as the penalties' l' and the constraint mask do,
 *               and everything downstream is defined on it in the words used above: the greedy pick, y = bf16(l / T) and its Gumbel
 *               key, the truncation classes, the token log-probabilities (renormalised), the top-n alternatives.
 *   order       a step is lm_head, [penalty], ngram ban, [constrain], step end, [top-logprobs], [advance]: HF's processor order.
 *   off         hist_len[b] < 0 is a row switched off: nothing recorded, nothing banned, no byte of the row written.
 *   full        a row whose history is full at record time (hist_len[b] == hist_ld) gets hist_len[b] = UMV_NGRAM_FULL and is off
 *               from then on; nothing is ever written at or beyond hist_ld.  (Callers size hist_ld so that this cannot happen: it is
 *               the kernel's defined behaviour, not a supported mode.)
 *   tiles       with argmax_partial every tile that holds a banned column carries the bits the lm_head epilogue of umv_gemm_bf16 would
 *               leave for the banned logits: greedy keys when temperature = 0, the sampling keys of (temperature, seed, *step)
 *               otherwise - with rows, of rows[b]'s temperature and (seed, draw, stream); lse_partial, when given, the statistics in
 *               epi_lse_tile's order.  A row with an empty ban set gets no write to its logits, keys or statistics.  argmax_partial =
 *               NULL: record and ban only (the unfused step).
 * umv_logit_ngram_ban_bf16: one workgroup per row, no word shared between workgroups; a row's result depends only on its own logits
 * and history.  UMV_ERR_ARG: what umv_logit_penalty_bf16 rejects of the fields the two share (temperature < 0 or not finite,
 * lse_partial without argmax_partial, n_tiles that is not ceil(V / 16) with argmax_partial, rows with a scalar temperature other than
 * 0, a misaligned table), a NULL hist, hist_len or ids, hist_ld < 1, a scalar n < 0 or > UMV_NGRAM_MAX. */
#define UMV_NGRAM_MAX 16
#define UMV_NGRAM_FULL (-2)
typedef struct {
    uint16_t* logits;          /* [M][V] bf16, row stride ld elements; banned in place */
    int64_t ld;
    const int64_t* ids;        /* [M]: the token each row is fed at this step */
    int32_t* hist;             /* [M][hist_ld] */
    int64_t hist_ld;
    int32_t* hist_len;         /* [M]; negative = the row is off */
    const int32_t* row_n;      /* optional [M]: the size of each row; NULL = the scalar n for all */
    int M, V;
    int n;                     /* 0 = record only */
    float temperature;         /* as given to the lm_head GEMM: 0 = greedy keys and y = l */
    uint64_t* argmax_partial;  /* optional [M][n_tiles] */
    float* lse_partial;        /* optional [M][n_tiles][2], only with argmax_partial */
    int n_tiles;
    uint64_t seed;             /* sample_seed / sample_step of the lm_head call (temperature > 0) */
    const int64_t* step;
    const umv_row_sampling* rows; /* optional [M]: row b's temperature and (seed, draw, stream); the scalar temperature must be 0 */
} umv_ngram_ban_args;
int umv_logit_ngram_ban_bf16(const umv_ngram_ban_args* a, umv_stream_t stream);

/* ------------------------------------------------------------------ speculative greedy decode: verify drafts, commit, roll back, draft again
 * A step of k = draft_len >= 1 processes T = B * (k + 1) <= 64 rows.  Row r0 = b * (k + 1) holds sample b's next input token t0, which is
 * not in the cache yet; rows r0 + j, j = 1..k, hold its drafts d_j: the first n_draft[b] are real, the rest are FILLERS equal to t0 -
 * computed, never accepted.  Before the step, tok_slot[r0 + j] = slot0 + j, tok_pos[r0 + j] = pos0 + j and kv_len[b] = len + k + 1, so that
 * umv_qkv_post appends all k + 1 tokens and umv_attn_varlen (max_q = k + 1, causal) lets row j see the keys 0..len + j.  After the greedy
 * lm_head call (argmax_partial [T][n_tiles], sample_temperature = 0) this entry ends the step, one workgroup per sample, no word shared
 * between workgroups.  All of it is integer logic, so the definition is exact:
 *   1 pick     p_j = column of the maximum key of argmax_partial[r0 + j][0..n_tiles), j = 0..k (umv_decode_step_end_argmax's pick).
 *   2 accept   n = the largest n <= n_draft[b] with d_j == p_{j-1} for all 1 <= j <= n.
 *   3 emit     m = min(n + 1, min(limit[b], out_ld) - n_out[b]), at least 0: out_ids[b][n_out[b] + i] = p_i, i < m; n_out[b] += m.
 *   4 advance  slot0, pos0 and kv_len[b] go up by m: the cache now holds t0, d_1..d_{m-1}.  The K/V of the rejected rows lies above
 *              the new length and is overwritten by the next step, which writes the slots len..len + k: a rollback is this shorter length.
 *   5 history  the m emitted tokens are appended to hist[b] (int32 [B][hist_ld]; hist_len[b] += m; a token that finds no room below
 *              hist_ld is dropped and hist_len[b] stays at hist_ld - later drafts get worse, the output does not change).  If m > 0
 *              the next input is p_{m-1}, else it stays t0.
 *   6 draft    by one of two rules; a draft is always a token of [0, V):
 *              predicted continuation, for a sample with predicted != NULL and pred_len[b] > 0 (predicted int64 [B][pred_ld] is
 *                aligned with out_ids): d_j = predicted[b][n_out[b] + j - 1], j = 1..k, while that index is < pred_len[b] and the
 *                entry is in [0, V);
 *              prompt lookup otherwise: for g = ngram_max down to ngram_min with hist_len[b] > g, the suffix is the last g history
 *                tokens; the match is the largest i < hist_len[b] - g with hist[b][i..i + g) equal to the suffix, entries < 0 (the
 *                caller's separators) never match.  The FIRST g that has a match decides: d_j = hist[b][i + g + j - 1], j = 1..k,
 *                while the index is < hist_len[b] and the entry is in [0, V).  No match for any g: no drafts.
 *              n_draft[b] = how many that gave.
 *   7 rows     ids[r0] = the next input, ids[r0 + j] = d_j (fillers: the next input), tok_slot[r0 + j] = slot0 + j,
 *              tok_pos[r0 + j] = pos0 + j for j = 0..k.
 *   8 stats    stats[b] = {steps, drafted, accepted} (int32 x 3) += {1, the n_draft[b] this step verified, n}.
 * draft_only != 0 runs 6 and 7 alone (nothing is read from argmax_partial, which may be NULL): the call that seeds the first step's rows
 * from the history / the predicted continuation.  UMV_ERR_ARG: k < 1, B * (k + 1) > 64, ngram_min < 1 or ngram_min > ngram_max, V that
 * is not the column count behind n_tiles, a NULL required pointer (everything but predicted / pred_len, which go together). */
typedef struct {
    int32_t* tok_slot;               /* [T] */
    int32_t* tok_pos;                /* [T] */
    int32_t* kv_len;                 /* [B] */
    const uint64_t* argmax_partial;  /* [T][n_tiles] */
    int n_tiles;
    int V;
    int64_t* ids;                    /* [T]: this step's rows in, the next step's out */
    int64_t* out_ids;                /* [B][out_ld] */
    int64_t out_ld;
    int32_t* n_out;                  /* [B] */
    const int32_t* limit;            /* [B]: emit no token at or beyond out_ids[b][limit[b]] */
    int32_t* n_draft;                /* [B] */
    int32_t* hist;                   /* [B][hist_ld] */
    int64_t hist_ld;
    int32_t* hist_len;               /* [B] */
    const int64_t* predicted;        /* optional [B][pred_ld] */
    int64_t pred_ld;
    const int32_t* pred_len;         /* [B], with predicted */
    int32_t* stats;                  /* [B][3] */
    int B, k, ngram_min, ngram_max, draft_only;
} umv_spec_step_args;
int umv_decode_step_end_speculative(const umv_spec_step_args* a, umv_stream_t stream);

/* ------------------------------------------------------------------ speculative decode with sampling: verify drafts against the seeded draw
 * A request's noise is keyed by its own (seed, stream, draw) - "per-row sampling parameters" - not by the step or the row it sits in, so
 * token i of a request is a fixed function of the logits its prefix produces and of draw = i.  A speculative step therefore gives row
 * r0 + j of sample b a table entry with the sample's parameters, seed and stream and draw = d0 + j (d0 = the number of tokens emitted so
 * far): the lm_head epilogue (the per-row call over T = B * (k + 1) rows) and the pick below then produce, for that row, exactly the token
 * the plain per-row step would pick after the prefix t0, d_1..d_j, and draft d_{j+1} is accepted exactly when it equals that pick.  No
 * rejection-sampling arithmetic and no residual distribution: a deterministic draft is accepted with the probability the (truncated)
 * softmax gives it, and the emitted sequence is the plain per-row session's, token for token (up to the last bit of a logit: the
 * attention's key split depends on the segment length).  A greedy row (temperature <= 0) is the greedy speculative step's row.
 * The step ends in two launches:
 *
 * umv_decode_pick_rows: one workgroup per ROW, T <= 64.  The pick part of umv_decode_step_end_rows with the row's own values, and
 * nothing else: picks[r] (int64) = the truncated pick on a sampled row with a filter on (the fused pick if it survived, else the kept
 * set's Gumbel maximum with regenerated noise), the key maximum otherwise; logprob[r] (fp32, with lse_partial or neither) = the pick's
 * own log-probability, the statistics merged in the order umv_decode_step_end_rows uses for that kind of row (NaN for a pick outside
 * [0, V)); cut_y[r] / n_kept[r] (optional) = the row's cutoff and kept count (-inf / V without a filter).  It advances no slot,
 * position or length and only READS the table.  UMV_ERR_ARG as umv_decode_step_end_rows has it, plus T > 64 and a NULL picks.
 *
 * umv_decode_step_end_speculative_rows: steps 2-8 of "speculative greedy decode" unchanged, one workgroup per sample, with
 *   1 pick     p_j = picks[r0 + j] (what umv_decode_pick_rows left) instead of the key maxima; step.argmax_partial is not read;
 *   9 draws    with d0 = rows[r0].draw before the step and m the number emitted: rows[r0 + j].draw = d0 + m + j, j = 0..k - so m = 0
 *              leaves the draws alone.  The only words of the table the launch writes;
 *   logprobs   with row_logprob [T] and out_logprobs [B][step.out_ld] (both or neither): out_logprobs[b][n_out + i] = row_logprob[r0 + i]
 *              for the m emitted tokens (n_out before the step).
 * step.draft_only != 0 touches neither the table nor the log-probabilities (the host packs the first draws).  UMV_ERR_ARG: what
 * umv_decode_step_end_speculative refuses (argmax_partial may be NULL), a NULL picks (unless draft_only), a NULL or misaligned table,
 * row_logprob without out_logprobs or the reverse. */
int umv_decode_pick_rows(const uint64_t* argmax_partial, const float* lse_partial, int n_tiles, const uint16_t* logits, int64_t ldo, int V,
                         const umv_row_sampling* rows, int T, int64_t* picks, float* logprob, float* cut_y, int32_t* n_kept,
                         umv_stream_t stream);
typedef struct {
    umv_spec_step_args step;         /* as for umv_decode_step_end_speculative; argmax_partial is not read */
    const int64_t* picks;            /* [T] */
    umv_row_sampling* rows;          /* [T]: only `draw` is written */
    const float* row_logprob;        /* optional [T] */
    float* out_logprobs;             /* optional [B][step.out_ld], with row_logprob */
} umv_spec_rows_step_args;
int umv_decode_step_end_speculative_rows(const umv_spec_rows_step_args* a, umv_stream_t stream);

/* ------------------------------------------------------------------ beam search decode
 * K beams per request, 2 <= K <= UMV_BEAM_K_MAX (K = 1 is greedy decode and runs the plain step): a step has R = B * K ordinary rows,
 * row b * K + i beam i of request b, each its own segment of a paged KV cache.  tests/beam_ref.py is this text in plain Python.
 * Each live beam has an fp32 score s_i, [0, -inf, ..., -inf] at the start: all K rows start from one prompt and one start token.
 * Step t = 0, 1, ... works on the rows' logits in this order:
 *  1. Candidates.  The first n = 2K columns of every row in the top-n order above - y descending, column ascending, y the bf16 logit
 *     (greedy definition) - each with lp = (y - ref) - logf(S) as the top-n alternatives define it, (ref, S) merged from lse_partial
 *     in the greedy step end's order (umv_decode_step_end_logprob): a row's list is its umv_decode_top_logprobs list bit for bit.
 *     total = s_i + lp, one fp32 add.  A beam whose s_i is not above -inf contributes nothing, nor does an id of -1 (a NaN row).
 *  2. Order.  All candidates of the request by (total descending, beam ascending, place in the beam's own list ascending); r is a
 *     candidate's place in that order.  Restricting each beam to its own 2K best does not change the first 2K of the full K * V order.
 *  3. Walk in that order until K live successors are found.  A candidate whose token is end_token_id is a finished hypothesis if
 *     r < K and is skipped otherwise; it never becomes a live beam.  Every other candidate becomes the next live beam, in order,
 *     with (token, parent beam, total, lp).  V > 2K, so that K other candidates exist (a beam's list holds the end token once).
 *     At the LAST step, t + 1 == max_len, every candidate with r < K is a finished hypothesis, whatever its token: this is how the
 *     live beams are offered at max_length (HF generate: the length criterion ends every candidate of that step; only the first K
 *     count).  A hypothesis' normalised score is total / norm[t], norm[t] = powf(t + 1, length_penalty) computed by the host in
 *     fp32 (len_norm): t + 1 is its number of generated tokens, the end token counted; the one fp32 division is the device's.
 *  4. Finished list, at most K entries.  While there is room an entry is appended; a full list replaces its worst entry - lowest
 *     score, the latest among equals - only for a strictly better one.  An entry is fin_f (score, total, lp of its last token, 0)
 *     and fin_i (step, parent beam = back-pointer into step - 1, last token, sequence number of the entry).
 *  5. Done.  early_stopping: the request is done when its list is full.  Otherwise: when the list is full AND its worst score is
 *     >= (best new live total) / norm[t] (HF's early_stopping=False heuristic, current length).  A done request's words are never
 *     written again: its workgroup returns at once, its rows go on computing and are ignored.
 *  6. The host takes the best hypothesis: highest score, the earlier entry among equals.
 *
 * KV plan.  L = the request's committed length after the step (tok_slot + 1), j0 = prompt length / 256.  Entries below j0 of a row's
 * table row are the shared prompt pages.  From j0 on every row owns TWO private pages per page index (own [R][n_own][2], index
 * j0 + q): the one its table row names and a spare.  Child c of parent p: entries j0 <= j < L / 256 (full pages) become
 * table_old[p][j], a pointer only; if L % 256 != 0 and p != c, copies[c] = (table_old[p][L / 256], c's spare of that index,
 * L % 256 rounded up to 8) and c's entry flips to the spare - sources are current pages, destinations spares, so a swap of two beams
 * never overwrites its own source; slots at or above L hold nothing committed.  Otherwise copies[c] = (0, 0, 0).  The workgroup reads
 * every table word it changes, barriers, then writes; no other workgroup touches its rows.  In the step that sets done, the table
 * stays and the copies are (0, 0, 0).  So: the page a row appends to next is referenced by no other row; no page below a live row's
 * length is written; only the fork's private pages are written.
 *
 * umv_beam_candidates: one workgroup of 512 threads per row, cand_ids (int32) / cand_lp (fp32) [R][n], rank [R] scratch (0).
 * umv_beam_step_end: one workgroup per request, steps 2-5, the next ids, the back-pointers beam_tok / beam_parent / beam_lp row t, the
 *   scores, slot / position / kv_len / step counter + 1 for the request's rows, the table rows and the copy list.  hdr [B][4] =
 *   (entries in the list, entries ever, done, 0).  K * n_own <= UMV_BEAM_TABLE_ENTRIES.  UMV_ERR_ARG: a NULL pointer, K outside
 *   [1, UMV_BEAM_K_MAX], misaligned copies / hdr.
 * umv_beam_kv_copy: grid (chunk, layer, row); pools [2 * layers] device pointers, K pool then V^T pool of each layer; for each kv head
 *   K [tokens][hd] and V^T [hd][tokens] go from the source page to the destination page in 16-byte accesses (hd % 8 == 0).  A row
 *   with tokens = 0 leaves at its first branch; a page outside [0, npages) copies nothing. */
#define UMV_BEAM_K_MAX 10
#define UMV_BEAM_TABLE_ENTRIES 1024
typedef struct {
    int32_t* tok_slot;               /* [R] */
    int32_t* tok_pos;                /* [R] */
    int32_t* kv_len;                 /* [R] */
    int64_t* ids;                    /* [R]: the tokens the next step is fed */
    int64_t* step_idx;               /* [R]: one counter per row, all equal */
    const int32_t* cand_ids;         /* [R][2K] */
    const float* cand_lp;            /* [R][2K] */
    float* scores;                   /* [R] */
    int32_t* beam_tok;               /* [max_len][R] */
    int32_t* beam_parent;            /* [max_len][R] */
    float* beam_lp;                  /* [max_len][R] */
    float* fin_f;                    /* [B][K][4] */
    int32_t* fin_i;                  /* [B][K][4] */
    int32_t* hdr;                    /* [B][4] */
    const float* len_norm;           /* [max_len] */
    int32_t* table;                  /* the page table rows of the R segments */
    const int32_t* own;              /* [R][n_own][2] */
    const int32_t* j0;               /* [B] */
    int32_t* copies;                 /* [R][4]: source page, destination page, tokens, 0 */
    int32_t table_stride, n_own, B, K, max_len, end_token_id, early_stopping;
} umv_beam_step_args;
int umv_beam_candidates(const uint16_t* logits, int64_t ldo, int V, const float* lse_partial, int n_tiles, int R, int n, int32_t* cand_ids,
                        float* cand_lp, int32_t* rank, umv_stream_t stream);
int umv_beam_step_end(const umv_beam_step_args* a, umv_stream_t stream);
int umv_beam_kv_copy(const int32_t* copies, const void* const* pools, int R, int layers, int nkv, int hd, int npages, int chunks,
                     umv_stream_t stream);

/* ------------------------------------------------------------------ banned sequences
 * bad_words_ids, suppress_tokens, begin_suppress_tokens and min_new_tokens: a row may not emit a token that would complete a listed
 * sequence, and some entries hold only for a row's first tokens.  tests/sequence_ban_ref.py is this text in plain Python.
 *   table       S entries, 0 <= S <= UMV_SEQ_ENTRIES_MAX, in CSR form in device memory: entry s is the token sequence
 *               w[0..m) = seq_tok[seq_ptr[s] .. seq_ptr[s + 1]), 1 <= m <= UMV_SEQ_MAX, n_tok = seq_ptr[S] tokens in all, with the word
 *               until = seq_until[s]:  0 = always active;  u > 0 = active only while the row's count <= u;  UMV_SEQ_ROW (-1) = active
 *               while count <= row_min[b] (a row value of 0 is never active, a NULL row_min is never active).  Any other until
 *               word, or an entry whose length or offsets are outside the table, is never active (the host validates them: the table
 *               is caller memory).
 *   history     row b owns count[b], the number of tokens it has been fed since its slot started, after this step's record, and
 *               tail [M][UMV_SEQ_MAX - 1], the last 15 tokens fed, most recent last, -1 where there is none.  The kernel records the
 *               token the step is fed, ids[b] - the start token and forced tokens included; an id outside [0, 2^31) is recorded as
 *               -1 (the n-gram kernel's rule).  A slot starts with count 0 and a tail of -1; the count stops at 2^31 - 1.
 *   off         count[b] < 0 is a row switched off: nothing recorded, nothing banned, no byte of the row written.
 *   banned set  entry s bans column w[m - 1] when it is active, m - 1 <= count, the last m - 1 history tokens equal w[0..m - 1)
 *               element for element, and w[m - 1] lies in [0, V).  A -1 or out-of-range token - in the history or in w[0..m - 1) -
 *               matches nothing.
 *   column      a banned column becomes bf16 -inf (0xFF80), also where it held NaN; every other column keeps its bits.  A row with an
 *               empty banned set gets no write to its logits, keys or statistics.
 *   tiles       with argmax_partial (and optionally lse_partial) every tile that holds a banned column carries the bits the lm_head
 *               epilogue would leave for the banned logits, exactly as umv_logit_ngram_ban_bf16 leaves them: scalar (temperature,
 *               seed, *step) or the per-row table rows.  argmax_partial = NULL: record and ban only (the unfused step).
 *   order       a step is lm_head, [penalty], [ngram ban], sequence ban, [constrain], step end, ...  All three bans store -inf and
 *               commute; the penalties keep -inf.
 *   HF          bad_words_ids=[w...] = entries (w, 0); suppress_tokens=[t...] = ([t], 0); begin_suppress_tokens=[t...] = ([t], 1);
 *               min_new_tokens=n with end token e = ([e], UMV_SEQ_ROW) and row_min[b] = n.  The history is the fed tokens only, start
 *               token first: a bad word that begins in the prompt is out of scope.  (HF skips a word longer than its whole input; here a word
 *               whose first m - 1 tokens ARE everything fed so far, start token included, bans - a start token no word holds, or
 *               a prompt in HF's input, makes the two the same.)
 *   beam form   K >= 1: the same kernel without tail / count, recording nothing.  Row r = b * K + i at step t = step_idx[r] has
 *               count = t + 1 and the tail ids[r], then beam_tok[u][b * K + i_u] for u = t - 2, t - 3, ..., with
 *               i_{t-2} = beam_parent[t - 1][r] and i_{u-1} = beam_parent[u][b * K + i_u] (beam_tok / beam_parent [max_len][M] of
 *               umv_beam_step_end; parents are beam indices inside the request), then the request's start token start_ids[b] before
 *               u = 0.  The walk reads max_m - 1 tokens, max_m the longest entry's length as the caller states it (longer entries
 *               see -1 beyond and do not match): max_m = 1 walks nothing.  A step counter outside [0, max_len) or a parent outside
 *               [0, K) ends the walk (the rest of the tail is -1; the former bans nothing).  The beam form is greedy: rows is NULL.
 * umv_logit_sequence_ban_bf16: one 256-thread workgroup per row, no word shared between workgroups.  UMV_ERR_ARG: what
 * umv_logit_ngram_ban_bf16 rejects of the shared fields; S outside [0, UMV_SEQ_ENTRIES_MAX]; NULL seq_ptr / seq_tok / seq_until with
 * S > 0; n_tok < S or > S * UMV_SEQ_MAX; max_m outside [0, UMV_SEQ_MAX] (or 0 with S > 0); NULL ids; the plain form (K = 0) without
 * tail / count; the beam form without beam_tok / beam_parent / step_idx / start_ids, with K outside [1, UMV_BEAM_K_MAX], M no
 * multiple of K, max_len < 1, or with rows.  A rejected call launches nothing. */
#define UMV_SEQ_MAX 16
#define UMV_SEQ_ENTRIES_MAX 4096
#define UMV_SEQ_ROW (-1)
typedef struct {
    uint16_t* logits;          /* [M][V] bf16, row stride ld elements; banned in place */
    int64_t ld;
    const int64_t* ids;        /* [M]: the token each row is fed at this step */
    const int32_t* seq_ptr;    /* [S + 1] */
    const int32_t* seq_tok;    /* [n_tok] */
    const int32_t* seq_until;  /* [S] */
    const int32_t* row_min;    /* optional [M] */
    int32_t* tail;             /* plain form: [M][UMV_SEQ_MAX - 1] */
    int32_t* count;            /* plain form: [M]; negative = the row is off */
    const int32_t* beam_tok;   /* beam form: [max_len][M] */
    const int32_t* beam_parent;/* beam form: [max_len][M] */
    const int64_t* step_idx;   /* beam form: [M] */
    const int64_t* start_ids;  /* beam form: [M / K], one per request */
    int M, V, S, n_tok, max_m;
    int K;                     /* 0 = the plain form; >= 1 = the beam form with K beams per request */
    int max_len;               /* beam form */
    float temperature;         /* as given to the lm_head GEMM: 0 = greedy keys and y = l */
    uint64_t* argmax_partial;  /* optional [M][n_tiles] */
    float* lse_partial;        /* optional [M][n_tiles][2], only with argmax_partial */
    int n_tiles;
    uint64_t seed;             /* sample_seed / sample_step of the lm_head call (temperature > 0) */
    const int64_t* step;
    const umv_row_sampling* rows; /* optional [M]: row b's temperature and (seed, draw, stream); the scalar temperature must be 0 */
} umv_sequence_ban_args;
int umv_logit_sequence_ban_bf16(const umv_sequence_ban_args* a, umv_stream_t stream);

/* ------------------------------------------------------------------ classifier-free guidance for text
 * HF's guidance_scale (UnbatchedClassifierFreeGuidanceLogitsProcessor) on the stored logits of a decode step: a CONDITIONAL row is
 * contrasted with an UNCONDITIONAL row of the same step - the same prompt without its images (visual contrastive decoding), or a
 * negative prompt.  A step has M rows; pair [M] (int32, device memory) names for a guided row c its unconditional row u = pair[c].
 *   active    row c is ACTIVE when u = pair[c] lies in [0, M), u != c, scale[c] is finite, >= 0 and not exactly 1 (HF returns
 *             log_softmax there: the same distribution), pair[u] does not itself name a row of [0, M) other than u (a row is never
 *             both guided and read), and no row c' < c has pair[c'] == u (an unconditional row serves one guided row).  Every other
 *             row - pair[r] = -1 is the way to say so - is left untouched in every bit, its keys and statistics included.  The
 *             host refuses tables that break the last two rules; the kernels only hold to them.
 *   lse       a row r TAKES PART when it is active or the u of an active row.  For such a row lse[r] = M_r + logf(S_r) and
 *             row_max[r] = M_r, where (M_r, S_r) is the merge, in the order of the step ends (one 256-thread workgroup: thread-strided,
 *             the wave tree, waves 0..3), of the per-tile (max, sum exp) of the stored bf16 logits l at temperature 0 - the tile
 *             pairs in the lm_head epilogue's order.  HF runs this processor before the temperature warper, so no temperature is
 *             applied here.  Where the lm_head call left lse_partial at temperature 0 (or 1: y = l there too) those ARE the tile
 *             pairs; otherwise the call first writes them to `stats` [M][n_tiles][2].  A -inf column adds 0; a NaN logit makes
 *             lse[r] NaN; M_r is the maximum over the columns that are not NaN.  Rows that take no part get no write to lse / row_max.
 *   column    for an active row c with g = scale[c], in fp32, one rounding per operation, nothing contracted to an FMA:
 *                 if l_c[n] == -inf or l_c[n] < M_c + log_beta[c]:   l'[n] = -inf      (banned stays banned; the plausibility floor)
 *                 else  cc = l_c[n] - lse[c]
 *                       if l_u[n] == -inf:                           l'[n] = bf16(cc)  (the unconditional row has no opinion)
 *                       else  uu = l_u[n] - lse[u];  d = cc - uu;  a = g * d;  a = a + uu;  l'[n] = bf16(a)
 *             = HF's scale * (cond - uncond) + uncond on log-softmaxes.  A NaN in either operand gives NaN through the arithmetic.
 *             log_beta[c] = logf(beta), beta in [0, 1) the plausibility floor of contrastive decoding (-inf = off = HF exactly): the
 *             columns the conditional row itself finds implausible are dropped, the maximum column always survives.  An active row
 *             whose M_c is -inf is left as it is.  l' REPLACES l in the conditional row; the unconditional row is only read.
 *   tiles     with argmax_partial (and lse_partial when given) EVERY tile of a rewritten row holds the bits the lm_head epilogue
 *             leaves for l': greedy keys at temperature 0, the sampling keys of (temperature, seed, *step) otherwise, the statistics
 *             of pick_value(l', temperature).  Whatever follows - penalties, bans, the step ends, the top-n alternatives - is
 *             defined on l'.  argmax_partial = NULL: the logits only.
 *   order     the stage is the FIRST behind the lm_head call: lm_head, guidance, [penalty], [bans], [constrain], step end, ...,
 *             guidance feed (HF's processor order).
 * umv_logit_guidance_bf16: up to three launches on one stream - the tile pairs (grid (UMV_CONSTRAIN_CHUNK columns, row), only when
 * lse_partial cannot serve), the merge (one workgroup per row), the combine (grid (UMV_CONSTRAIN_CHUNK columns, row), one tile per
 * thread).  No word is shared between workgroups of a launch; a pair's result does not depend on the batch it sits in.  UMV_ERR_ARG:
 * NULL logits / pair / scale / log_beta / lse / row_max, ld < V, temperature < 0 or not finite, lse_partial without argmax_partial,
 * n_tiles that is not ceil(V / 16), no lse_partial at temperature 0 or 1 and no stats either, M > 65535.  M = 0 is UMV_OK.  The
 * per-row arrays live in device memory so that a slot can be re-pointed between replays of a captured step.
 *
 * umv_guidance_feed: one launch BEHIND the step end (umv_decode_step_end_argmax / _logprob / _truncated), one thread per row.  For
 * every row c whose pair word passes the rules above (the scale is not looked at: a pair at scale 1 still decodes in lockstep) the
 * token the step end left for c becomes u's: ids[u] = ids[c], and with s = step_idx[c] - 1 the step just ended, pred_ids[s][u] =
 * pred_ids[s][c] (s in [0, max_len)) and in_ids[s + 1][u] = in_ids[s + 1][c] (s + 1 in [0, max_len)).  Nothing else is written:
 * u's slot, position, length and step counter advanced on their own. */
typedef struct {
    uint16_t* logits;          /* [M][V] bf16, row stride ld elements; active rows rewritten in place */
    int64_t ld;
    int M, V;
    const int32_t* pair;       /* [M]: the unconditional row of row c, -1 = not guided */
    const float* scale;        /* [M]: guidance_scale of row c */
    const float* log_beta;     /* [M]: logf(guidance_plausibility) of row c, -inf = off */
    float* lse;                /* [M] out: lse[r] of the rows that take part */
    float* row_max;            /* [M] out: M_r of the rows that take part */
    float* stats;              /* [M][n_tiles][2] workspace for the temperature-0 tile pairs; may be NULL where lse_partial serves */
    float temperature;         /* as given to the lm_head GEMM: 0 = greedy keys and y = l' */
    uint64_t* argmax_partial;  /* optional [M][n_tiles] */
    float* lse_partial;        /* optional [M][n_tiles][2], only with argmax_partial */
    int n_tiles;
    uint64_t seed;             /* sample_seed / sample_step of the lm_head call (temperature > 0) */
    const int64_t* step;
} umv_logit_guidance_args;
int umv_logit_guidance_bf16(const umv_logit_guidance_args* a, umv_stream_t stream);
int umv_guidance_feed(const int32_t* pair, int64_t* ids, int64_t* in_ids, int64_t* pred_ids, const int64_t* step_idx, int M, int max_len,
                      umv_stream_t stream);


/* TimestepEmbedder.timestep_embedding (modeling_utils.py:87-109): out[r] = bf16(cat(cos(t[r] * freqs), sin(t[r] * freqs))),
 * out [n, 2*half]; freqs [half] fp32 = exp(-ln(10000) * i / half) from the caller.  The two linears + SiLU of the embedder
 * are umv_gemm_bf16 calls (UMV_EPI_SILU). */
int umv_timestep_embed(const float* t, const float* freqs, uint16_t* out, int n, int half, umv_stream_t stream);

/* ------------------------------------------------------------------ image head
 * CFG combine + renorm + Euler update (bagel.py:1173-1207, :983), bf16 rounding after each
 * op as the reference's bf16 tensors imply; x_t [N,D] fp32 updated in place.  v_* are
 * [T, D] bf16 (row stride ldv); rows[n] picks the latent rows; seg_off [nseg+1] delimits the
 * samples in n (norms are per sample).  renorm_type 0 global, 1 channel, 2 text_channel. */
int umv_cfg_renorm_euler(float* x_t, const uint16_t* v_t, const uint16_t* v_text, const uint16_t* v_img, int64_t ldv,
                         const int32_t* rows, const int32_t* seg_off, int nseg, float cfg_text_scale,
                         float cfg_img_scale, float renorm_min, int renorm_type, float dt, int D, umv_stream_t stream);

/* ------------------------------------------------------------------ VAE (FLUX autoencoder, autoencoder.py)
 * Activations are NHWC bf16 ([B,H,W,C], C % 8 == 0).  Convolution weights [Cout,Cin,k,k] are
 * permuted to [Cout,(ky,kx,ci)] and packed with umv_pack_weight_bf16 (N=Cout, K=k*k*Cin).
 * umv_conv2d_nhwc_bf16 = F.conv2d (+bias, + optional residual x + h of ResnetBlock/AttnBlock,
 * autoencoder.py:95,65) as an MFMA implicit GEMM:
 *   mode 0: stride 1, pad (k-1)/2            (autoencoder.py:76,78,80,138,167,214,238)
 *   mode 1: nearest 2x upsample then 3x3     (Upsample, autoencoder.py:116-118)
 *   mode 2: F.pad(0,1,0,1) then 3x3 stride 2 (Downsample, autoencoder.py:104-107): floor(H/2) x floor(W/2) outputs, so an input
 *           of one row or one column gives an empty result (UMV_OK, nothing written)
 * k is 3, or 1 with mode 0 (modes 1 and 2 with k = 1: UMV_ERR_UNSUPPORTED).  UMV_ERR_ARG: a NULL x / wp / out, Cin no positive
 * multiple of 8, Cout <= 0, a negative B, Hin or Win. */
int umv_conv2d_nhwc_bf16(const uint16_t* x, const uint16_t* wp, const uint16_t* bias, const uint16_t* residual,
                         uint16_t* out, int B, int Cin, int Hin, int Win, int Cout, int ksize, int mode,
                         umv_stream_t stream);
/* nn.GroupNorm(32, C, eps, affine) on bf16 with optional swish x*sigmoid(x) (autoencoder.py:34-35,
 * 43,75,77,166,237); deterministic two-level reduction through `workspace`. */
size_t umv_groupnorm_workspace_bytes(int B, int HW);
int umv_groupnorm_nhwc_bf16(const uint16_t* x, const uint16_t* gamma, const uint16_t* beta, uint16_t* out, void* workspace,
                            int B, int HW, int C, float eps, int swish, umv_stream_t stream);
/* [B,C,H,W] fp32 -> NHWC bf16 with channels zero padded to Cp (input of encoder.conv_in) */
int umv_nchw_f32_to_nhwc_bf16(const float* x, uint16_t* out, int B, int C, int H, int W, int Cp, umv_stream_t stream);
/* latent tokens [h*w, p*p*c] fp32 -> NHWC bf16 [h*p, w*p, c] with z/scale + shift
 * (inferencer.py:239-241 unpatchify + autoencoder.py:306) */
int umv_unpatchify_latent(const float* tokens, uint16_t* out, int h, int w, int p, int c, float scale, float shift,
                          umv_stream_t stream);
/* decoder output NHWC bf16 (first 3 of Cs channels) -> uint8 HWC: (x*0.5+0.5).clamp(0,1)*255,
 * truncating cast (inferencer.py:253-254) */
int umv_pixels_to_u8(const uint16_t* x, uint8_t* out, int64_t npix, int Cs, umv_stream_t stream);
/* AttnBlock.attention (autoencoder.py:50-62: one head of C channels over H*W positions) as two umv_gemm_bf16 calls with fp32
 * outputs, S = Q K^T and O = P V, and these two row kernels between / after them (unimedvl_amd/vae.py::attnblock):
 *   umv_softmax_rows_f32:  P[r][c] = bf16(exp((S[r][c] - max_c S[r][c]) * scale)), l[r] = sum_c of the unrounded weights
 *                          (n even, <= 16384 columns; S [rows, ld_s] fp32, P [rows, ld_p] bf16)
 *   umv_rowscale_f32_bf16: out[r][c] = bf16(O[r][c] / l[r])
 * - the arithmetic of flash attention (fp32 scores and sums, bf16 weights, one division) with the row's true maximum. */
int umv_softmax_rows_f32(const float* S, int64_t ld_s, uint16_t* P, int64_t ld_p, float* l, int rows, int n, float scale,
                         umv_stream_t stream);
int umv_rowscale_f32_bf16(const float* O, int64_t ld_in, const float* l, uint16_t* out, int64_t ld_out, int rows, int C,
                          umv_stream_t stream);
/* encoder tail for sample b: moments NHWC [B,Hm,Wm,2z] + noise NCHW bf16 [B,z,Hm,Wm] ->
 * scale*(mean + exp(0.5*logvar)*noise - shift) (autoencoder.py:266-272,300-303), 2x2-patchified
 * tokens [h*w, p*p*z] of the top-left window (bagel.py:771-775) */
int umv_latent_sample_patchify(const uint16_t* moments, const uint16_t* noise, uint16_t* tokens, int b, int Hm, int Wm,
                               int z, int h, int w, int p, float scale, float shift, umv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
