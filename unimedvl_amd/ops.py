"""Thin torch-tensor wrappers over the C ABI (torch is used for device memory and
streams only).  Every function launches a hand-written gfx950 kernel from
libunimedvl_hip.so on torch's current stream; there is no fallback path."""
import ctypes as C
import functools

import torch

from . import _lib
from ._lib import (EPI_BIAS, EPI_GELU_TANH, EPI_OUT_F32, EPI_RESIDUAL, EPI_SILU, EPI_SWIGLU, AttnArgs, GemmArgs,
                   LogitConstrainArgs, LogitPenaltyArgs, NgramBanArgs, QkvPostArgs, TokenAutomatonArgs, check)

BF16 = torch.bfloat16


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """hipStream_t of torch's current stream on the current device (every op launches there)."""
    if _raw_stream is not None:       # ~0.3 us instead of ~3 us for building a torch.cuda.Stream object per launch
        return C.c_void_p(_raw_stream(torch.cuda.current_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def on_device(fn):
    """Method decorator: run with `self.device` as torch's current device.  Every kernel launches on the CURRENT device's
    current stream (_stream), so an engine built on cuda:N (the scripts' target_gpu_device, interactive_vqa_inferencer.py:60)
    must make N current around its public entry points; a no-op when it already is."""
    @functools.wraps(fn)
    def wrapper(self, *args, **kwargs):
        dev = torch.device(self.device)
        if dev.type != "cuda" or dev.index is None or dev.index == torch.cuda.current_device():
            return fn(self, *args, **kwargs)
        with torch.cuda.device(dev):
            return fn(self, *args, **kwargs)
    return wrapper


def device_scope(device):
    """Context manager form of on_device (constructors, where self.device does not exist yet)."""
    dev = torch.device(device)
    if dev.type != "cuda" or dev.index is None:
        import contextlib
        return contextlib.nullcontext()
    return torch.cuda.device(dev)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _req(t, dtype, name):
    if not t.is_cuda:
        raise _lib.UmvError(f"{name}: tensor must live on the GPU (no CPU fallback)")
    if t.dtype != dtype:
        raise _lib.UmvError(f"{name}: expected {dtype}, got {t.dtype}")
    return t


Z13_MAX_ROWS = 32      # rows up to which a linear's exact 13-bit image is streamed instead of its bf16 image (measured at 8 and 32)


class PackedLinear:
    """nn.Linear weight [N,K] (+bias) re-tiled for the MFMA GEMM kernels."""

    __slots__ = ("wp", "bias", "N", "K", "swiglu", "th", "w8", "scale", "w8m", "w4", "wz")

    def __init__(self, wp, bias, N, K, swiglu=False, th=16, w8=None, scale=None, w4=None):
        self.wp, self.bias, self.N, self.K, self.swiglu, self.th = wp, bias, N, K, swiglu, th
        # fp8 weights (BASELINE.json configs[4]): w8 = e4m3 image streamed by the decode GEMM (M <= 64), scale = its
        # power-of-two channel scales; wp is then the bf16 image of the SAME dequantised weights for M > 64
        self.w8, self.scale = w8, scale
        # optional: the e4m3 image re-tiled for the fp8 matrix instruction; when present, GEMMs with M > 64 rows quantise
        # their activations per row and run W8A8 (enable_fp8_mfma)
        self.w8m = None
        # MXFP4 weights (llm_weight_dtype="fp4"): w4 = the e2m1 + block-scale image, streamed by the decode GEMM (M <= 64) and read by
        # the tiled MXFP4 GEMM above that; wp is then either the bf16 image of the SAME dequantised weights (M > 64 runs on it when it is
        # there: bit-identical) or None (keep_bf16=False / drop_bf16: the linear stands on its 4-bit image alone)
        self.w4 = w4
        # optional: the exact 13-bit image of wp (build_z13), streamed instead of wp by the decode forms of the GEMM (SwiGLU, argmax keys,
        # split-K partials) up to Z13_MAX_ROWS rows: same bits, 13/16 of the bytes; wp stays (its fallback, and every other GEMM)
        self.wz = None

    def build_z13(self):
        """Add the exact 13-bit image of the bf16 image (include/unimedvl_hip.h, "z13"): the decode forms of the GEMM then stream it."""
        if self.wp is None or self.th != 16 or self.w8 is not None or self.w4 is not None or self.K % 64 or self.K > 32768:
            raise _lib.UmvError("build_z13 needs a plain bf16 linear (16-row image) with K a multiple of 64, K <= 32768")
        lib = _lib.load()
        self.wz = torch.empty(lib.umv_packed_weight_z13_bytes(self.N, self.K), dtype=torch.uint8, device=self.wp.device)
        check(lib.umv_pack_weight_z13(_p(self.wp), _p(self.wz), self.N, self.K, _stream()), "umv_pack_weight_z13")
        return self

    def drop_bf16(self):
        """Release the bf16 image of the dequantised weights of an fp4 linear: M > 64 then runs the tiled GEMM on the MXFP4 image."""
        if self.w4 is None:
            raise _lib.UmvError("drop_bf16 needs MXFP4 weights (from_weight_mxfp4 / from_gate_up_mxfp4)")
        self.wp = None
        return self

    def enable_fp8_mfma(self, keep_bf16=False):
        """Build the fp8-MFMA image from the e4m3 image; the bf16 image of the dequantised weights is dropped unless asked."""
        if self.w8m is not None:        # already there (e.g. read back from the packed fast-path file)
            if not keep_bf16:
                self.wp = None
            return self
        if self.w8 is None:
            raise _lib.UmvError("enable_fp8_mfma needs fp8 weights (from_weight_fp8 / from_gate_up_fp8)")
        lib = _lib.load()
        self.w8m = torch.empty(lib.umv_packed_weight_fp8_mfma_bytes(self.N, self.K), dtype=torch.uint8, device=self.w8.device)
        check(lib.umv_repack_weight_fp8_mfma(_p(self.w8), _p(self.w8m), self.N, self.K, _stream()), "umv_repack_weight_fp8_mfma")
        if not keep_bf16:
            self.wp = None
        return self

    @staticmethod
    def _operands(w, up):
        """the checked weight of a plain linear (up = None) or the gate / up pair of a SwiGLU one, with rows per operand, N and K"""
        if up is None:
            w = _req(w.contiguous(), BF16, "weight")
        else:
            w, up = _req(w.contiguous(), BF16, "gate"), _req(up.contiguous(), BF16, "up")
            assert w.shape[0] % 16 == 0, "intermediate size must be a multiple of 16"
        rows, K = w.shape
        return w, up, rows, rows if up is None else 2 * rows, K

    @staticmethod
    def _bf16(w, up=None, bias=None):
        """the bf16 image of a plain linear, or of the interleaved SwiGLU pair gate = w / up"""
        lib = _lib.load()
        w, up, rows, N, K = PackedLinear._operands(w, up)
        wp = torch.empty(lib.umv_packed_weight_elems(N, K), dtype=BF16, device=w.device)
        if up is None:
            check(lib.umv_pack_weight_bf16(_p(w), _p(wp), N, K, _stream()), "umv_pack_weight_bf16")
        else:
            check(lib.umv_pack_weight_swiglu_bf16(_p(w), _p(up), _p(wp), rows, K, _stream()), "umv_pack_weight_swiglu_bf16")
        return PackedLinear(wp, None if bias is None else bias.contiguous(), N, K, swiglu=up is not None)

    @staticmethod
    def _quantized(fmt, w, up=None, bias=None, keep_bf16=True):
        """fmt "fp8" (e4m3, power-of-two channel scales) or "mxfp4" (e2m1, one power-of-two scale per 32 k): quantise, pack the
        dequantised copy with the bf16 constructor (keep_bf16=False: no such copy, not even as scratch), attach the image"""
        lib = _lib.load()
        w, up, rows, N, K = PackedLinear._operands(w, up)
        img = torch.empty(getattr(lib, f"umv_packed_weight_{fmt}_bytes")(N, K), dtype=torch.uint8, device=w.device)
        scale = torch.empty((N + 15) // 16 * 16, dtype=torch.float32, device=w.device) if fmt == "fp8" else None
        deq = torch.empty_like(w) if keep_bf16 else None
        deq_up = torch.empty_like(up) if keep_bf16 and up is not None else None
        images = (_p(img), _p(scale)) if fmt == "fp8" else (_p(img),)
        check(getattr(lib, f"umv_quantize_pack_weight_{fmt}")(_p(w), _p(up), *images, _p(deq), _p(deq_up), rows, K, _stream()),
              f"umv_quantize_pack_weight_{fmt}")
        if keep_bf16:
            lin = PackedLinear._bf16(deq, deq_up, bias)
        else:
            lin = PackedLinear(None, None if bias is None else bias.contiguous(), N, K, swiglu=up is not None)
        if fmt == "fp8":
            lin.w8, lin.scale = img, scale
        else:
            lin.w4 = img
        return lin

    @staticmethod
    def from_weight_fp8(w, bias=None):
        """Quantise an nn.Linear weight to e4m3 with power-of-two channel scales; see include/unimedvl_hip.h."""
        return PackedLinear._quantized("fp8", w, None, bias)

    @staticmethod
    def from_gate_up_fp8(gate, up):
        return PackedLinear._quantized("fp8", gate, up)

    @staticmethod
    def from_weight_mxfp4(w, bias=None, keep_bf16=True):
        """Quantise an nn.Linear weight to MXFP4 (e2m1, one power-of-two scale per 32 k); see include/unimedvl_hip.h.
        keep_bf16=False: no bf16 image of the dequantised weights is built (not even as scratch)."""
        return PackedLinear._quantized("mxfp4", w, None, bias, keep_bf16)

    @staticmethod
    def from_gate_up_mxfp4(gate, up, keep_bf16=True):
        return PackedLinear._quantized("mxfp4", gate, up, None, keep_bf16)

    @staticmethod
    def from_weight(w, bias=None):
        return PackedLinear._bf16(w, None, bias)

    @staticmethod
    def from_gate_up(gate, up):
        return PackedLinear._bf16(gate, up)

    def for_decode(self, n_cus=256):
        """A second, decode-only image with th-row tiles such that the number of tiles is a multiple of the
        CU count (exact partition of the weight stream over the chip); returns self when 16 is already fine."""
        if self.swiglu or self.th != 16 or self.w8 is not None or self.w4 is not None:
            return self
        best = None
        for th in range(15, 7, -1):
            if self.N % th == 0 and (self.N // th) % n_cus == 0:
                best = th
                break
        if best is None or ((self.N + 15) // 16) % n_cus == 0:
            return self
        lib = _lib.load()
        out = torch.empty(lib.umv_repacked_weight_elems(self.N, self.K, best), dtype=BF16, device=self.wp.device)
        check(lib.umv_repack_weight_rows_bf16(_p(self.wp), _p(out), self.N, self.K, best, _stream()), "umv_repack_weight_rows_bf16")
        return PackedLinear(out, self.bias, self.N, self.K, False, best)

    def nbytes(self):
        return self.wp.numel() * 2 if self.wp is not None else self.w4.numel()

    def decode_bytes(self):
        """bytes of the image a decode step (M <= 64) streams, by the rules of _route: the e4m3 or the MXFP4 image (block scales included)
        when there is one, else the exact 13-bit image (its few flagged blocks, which stream the bf16 image instead, are counted at 13
        bits), else the bf16 image"""
        for image in (self.w8, self.w4, self.wz):
            if image is not None:
                return image.numel()
        return self.wp.numel() * 2


def _z13_takes(lin, M, z13, form):
    """whether a call streams the linear's exact 13-bit image (the z13 step of _route).  form: "splitk" (split-K partials), "epilogue"
    (SwiGLU or argmax / sampling keys) or None (anything else).  z13 = None: the measured policy - split-K up to
    Z13_MAX_ROWS rows; the epilogue forms up to 8 rows and at 17..Z13_MAX_ROWS, not at 9..16, where gate/up and lm_head only tie with the
    bf16 kernel; True: whenever umv_gemm_z13w serves the call (M <= 64; tests, A/B); False: never"""
    if lin.wz is None or z13 is False:
        return False
    if z13:
        return M <= 64
    if form == "splitk":
        return M <= Z13_MAX_ROWS
    return form == "epilogue" and (M <= 8 or 16 < M <= Z13_MAX_ROWS)


def _route(lin, M, splitk=False, norm=False, amax=False, act8=False, out_f32=False, act=False, z13=None):
    """The one rule for which C entry point serves a GEMM call and on which image of the weight: (entry, image that goes into wp,
    w_scale, 13-bit image), or the error of a call that needs an image the linear does not have.  Reads what the linear holds and the
    call's form (split-K, norm_w / argmax_partial set, act8, out_f32, a GELU / SiLU epilogue, the z13 override), no tensor data.
    PackedLinear.decode_bytes counts the image the M <= 64 rules below pick."""
    if act8 and lin.w8m is None:
        raise _lib.UmvError("act8 needs a linear with the fp8-MFMA image (enable_fp8_mfma)")
    skinny = M <= 64 and not norm                   # a weight-streaming kernel can take the call
    if act8 and not splitk and M > 64 and not norm and not out_f32:
        return "umv_gemm_fp8a8w", lin.w8m, lin.scale, None     # W8A8: e4m3 activations per row, fp8 matrix instruction
    if lin.w8 is not None and (skinny or splitk):              # (split-K: whatever M - same split, same consumers)
        return "umv_gemm_fp8w", lin.w8, lin.scale, None
    if lin.w4 is not None:
        if skinny:
            return "umv_gemm_mxfp4w", lin.w4, None, None
        if lin.wp is None:                                     # no bf16 image of W': the tiled kernel on the MXFP4 image (split-K: same partials)
            if not splitk and (norm or amax):
                raise _lib.UmvError(f"this linear only has its fp4 (MXFP4) image (built with keep_bf16=False / drop_bf16): M={M} rows with "
                                    f"norm_w={'set' if norm else 'None'}, argmax_partial={'set' if amax else 'None'} need "
                                    "the bf16 kernel - build the weights with keep_bf16=True (llm_fp4_keep_bf16=True)")
            return "umv_gemm_mxfp4t", lin.w4, None, None
    if lin.wp is None and not splitk:
        raise _lib.UmvError(f"this linear only has fp8 images (the bf16 image was dropped by enable_fp8_mfma): M={M} rows with "
                            f"act8={act8}, out_f32={out_f32}, norm_w={'set' if norm else 'None'} need the bf16 kernel - "
                            "build the weights with enable_fp8_mfma(keep_bf16=True)")
    # the exact 13-bit image: the bf16 kernel's bits from 13/16 of the bytes.  Only the forms that were measured against the bf16 kernel
    # and won (_z13_takes): split-K down up to 32 rows, the SwiGLU gate/up GEMM and lm_head with the argmax /
    # sampling keys up to 8 and at 17..32 rows.  Every other call on such a linear - a short prefill, MoT text rows, down without a
    # split, plain lm_head, 33..64 rows, a fused norm, a GELU / SiLU epilogue - stays on umv_gemm_bf16.
    if _z13_takes(lin, M, z13, "splitk" if splitk else "epilogue" if (lin.swiglu or amax) else None) and not norm and not act:
        return "umv_gemm_z13w", lin.wp, None, lin.wz
    return "umv_gemm_bf16", lin.wp, None, None


def _launch(lib, route, x, lin, out, ldo, M, flags=0, residual=None, row_idx=None, norm_w=None, norm_eps=0.0, amax=None, sample=None,
            k_splits=0, split_stride=0, lse=None, sample_rows=None):
    """Build the umv_gemm_args of a routed call and launch it.  What only some entries take is set from the route: w_scale; th-row tiles
    and the bound on x's rows (the bf16 kernel and its 13-bit twin, outside split-K); the sampling mode (not the MXFP4 entries, which
    have no argmax keys); every other field is the call's"""
    entry, image, scale, wz = route
    a = GemmArgs(x=x.data_ptr(), ldx=x.stride(0), wp=None if image is None else image.data_ptr(), out=out.data_ptr(), ldo=ldo,
                 M=M, N=lin.N, K=lin.K, epilogue=flags, norm_eps=norm_eps, argmax_partial=amax)
    if flags & EPI_BIAS:
        a.bias = lin.bias.data_ptr()
    if residual is not None:
        a.residual, a.ldr = residual.data_ptr(), residual.stride(0)
    if row_idx is not None:
        a.row_idx = row_idx.data_ptr()
    if norm_w is not None:
        a.norm_w = norm_w.data_ptr()
    if scale is not None:
        a.w_scale = scale.data_ptr()
    if k_splits:
        a.k_splits, a.split_stride = k_splits, split_stride
    elif entry in ("umv_gemm_bf16", "umv_gemm_z13w"):
        a.tile_rows, a.x_rows = lin.th, x.shape[0]
    if sample is not None and entry not in ("umv_gemm_mxfp4w", "umv_gemm_mxfp4t"):
        a.sample_temperature, a.sample_seed, a.sample_step = _sample_fields(sample, amax)
    if lse is not None:
        a.lse_partial = lse
    if sample_rows is not None:         # the lm_head call with a per-row table: the entry's *_rows twin, the table behind the struct
        if wz is not None:
            check(lib.umv_gemm_z13w_rows(C.byref(a), wz.data_ptr(), sample_rows, _stream()), entry + "_rows")
        else:
            check(getattr(lib, entry + "_rows")(C.byref(a), sample_rows, _stream()), entry + "_rows")
    elif wz is not None:
        check(lib.umv_gemm_z13w(C.byref(a), wz.data_ptr(), _stream()), entry)
    else:
        check(getattr(lib, entry)(C.byref(a), _stream()), entry)
    return out


def gemm(x, lin, out=None, *, M=None, residual=None, act=None, row_idx=None, out_f32=False, use_bias=True,
         norm_w=None, norm_eps=1e-6, act8=False, argmax_partial=None, sample=None, z13=None, lse_partial=None, sample_rows=None):
    """out = epilogue(x @ W^T).  x [M,K] bf16 (row stride may exceed K).  act in {None,'gelu_tanh','silu'}.
    norm_w: fuse Qwen2RMSNorm(x)*norm_w into the GEMM prologue (M <= 16, K <= 4096).
    act8 (W8A8 mode, needs lin.w8m): the activations are rounded per row through e4m3 - on the fp8 matrix instruction for
    M > 64 rows, as a bf16 copy of the rounded rows for the weight-streaming kernels below that.
    argmax_partial (int64 [M, ceil(N/16)], M <= 64): greedy-argmax keys per 16-column tile, finished by decode_step_end_argmax.
    sample (with argmax_partial): (temperature, seed, step tensor or None) - the keys then order bf16(logit / T) + Gumbel noise, so the
    row maximum is one draw from softmax(logits / T) (bagel.py:1297-1299) instead of the greedy token.
    lse_partial (with argmax_partial; fp32 [M, ceil(N/16), 2]): per tile and row the maximum of the value the keys order without noise
    and the sum of exp(value - maximum) - the softmax statistics decode_step_end_logprob turns into the token's log-probability.  It
    rides on the argmax_partial epilogue: without argmax_partial the library refuses it (UMV_ERR_ARG).
    sample_rows (with argmax_partial, instead of sample; int64 [M, 6] = the per-row table of sampling.to_tensor): row m's keys and
    statistics are those of ITS temperature (0 = a greedy row) and (seed, draw, stream) - include/unimedvl_hip.h, per-row sampling
    parameters.  The bf16, 13-bit and e4m3 routes take it; the library refuses it without argmax_partial or above 64 rows.
    z13 (tests and A/B only; leave None): whether a linear's exact 13-bit image is streamed - None = the measured policy of _route,
    True = whenever umv_gemm_z13w serves the call, False = never."""
    lib = _lib.load()
    _req(x, BF16, "x")
    assert x.stride(-1) == 1
    M = x.shape[0] if M is None else M
    flags = 0
    if lin.bias is not None and use_bias:
        flags |= EPI_BIAS
    if act == "gelu_tanh":
        flags |= EPI_GELU_TANH
    elif act == "silu":
        flags |= EPI_SILU
    elif act is not None:
        raise ValueError(act)
    if lin.swiglu:
        flags |= EPI_SWIGLU
    if residual is not None:
        flags |= EPI_RESIDUAL
    if out_f32:
        flags |= EPI_OUT_F32
    if out is None:
        assert row_idx is None, "row-indexed GEMM writes into a caller-provided buffer"
        out = torch.empty((x.shape[0], lin.N // 2 if lin.swiglu else lin.N), dtype=torch.float32 if out_f32 else BF16, device=x.device)
    route = _route(lin, M, False, norm_w is not None, argmax_partial is not None, act8, out_f32, act is not None, z13)
    if act8 and M <= 64:
        x = fake_quantize_act(x, M, row_idx)
    if sample_rows is not None and route[0] not in ("umv_gemm_bf16", "umv_gemm_z13w", "umv_gemm_fp8w"):
        raise _lib.UmvError(f"gemm: sample_rows rides on the argmax_partial epilogue of the bf16 / 13-bit / e4m3 routes, not {route[0]}")
    amax = lse = rows = None
    if argmax_partial is not None or lse_partial is not None or sample_rows is not None:        # (a plain GEMM pays no call for them)
        amax, lse, rows, _ = _tile_keys("gemm", M, argmax_partial, lse_partial, sample_rows, (lin.N + 15) // 16)
    if route[0] == "umv_gemm_fp8a8w":
        if lse is not None:
            raise _lib.UmvError("gemm: lse_partial rides on the argmax_partial epilogue of the M <= 64 kernels")
        # W8A8: per-row e4m3 activations (rows gathered through row_idx), fp8 matrix instruction, exact pow2 scales
        xq, xs = quantize_act(x, M, row_idx, lin.K)
        a8 = _lib.Gemm8Args(xq=xq.data_ptr(), ldq=xq.stride(0), x_scale=xs.data_ptr(), wp=lin.w8m.data_ptr(), w_scale=lin.scale.data_ptr(),
                            out=out.data_ptr(), ldo=out.stride(0), M=M, N=lin.N, K=lin.K, epilogue=flags)
        if flags & EPI_BIAS:
            a8.bias = lin.bias.data_ptr()
        if residual is not None:
            a8.residual, a8.ldr = residual.data_ptr(), residual.stride(0)
        if row_idx is not None:
            a8.row_idx = row_idx.data_ptr()
        check(lib.umv_gemm_fp8a8w(C.byref(a8), _stream()), "umv_gemm_fp8a8w")
        return out
    return _launch(lib, route, x, lin, out, out.stride(0), M, flags, residual, row_idx, norm_w, norm_eps, amax, sample, lse=lse,
                   sample_rows=rows)


def rmsnorm(x, w, eps, out=None, w_gen=None, expert=None):
    lib = _lib.load()
    _req(x, BF16, "x")
    T, H = x.shape
    out = torch.empty_like(x) if out is None else out
    check(lib.umv_rmsnorm_bf16(_p(x), _p(w), _p(w_gen), _p(expert), _p(out), T, H, eps, _stream()), "umv_rmsnorm_bf16")
    return out


def layernorm(x, w, b, eps, out=None):
    lib = _lib.load()
    _req(x, BF16, "x")
    T, H = x.shape
    out = torch.empty_like(x) if out is None else out
    check(lib.umv_layernorm_bf16(_p(x), _p(w), _p(b), _p(out), T, H, eps, _stream()), "umv_layernorm_bf16")
    return out


def embed_gather(table, ids, out=None, out_rows=None):
    lib = _lib.load()
    _req(table, BF16, "table")
    _req(ids, torch.int64, "ids")
    T, H = ids.numel(), table.shape[1]
    if out is None:
        out = torch.empty((T, H), dtype=BF16, device=table.device)
    check(lib.umv_embed_gather_bf16(_p(table), _p(ids), _p(out_rows), _p(out), T, H, _stream()), "umv_embed_gather_bf16")
    return out


def add_rows(a, out, bcast=None, table=None, idx=None, out_rows=None):
    lib = _lib.load()
    _req(a, BF16, "a")
    T, H = a.shape
    check(lib.umv_add_rows_bf16(_p(a), _p(bcast), _p(table), _p(idx), _p(out_rows), _p(out), T, H, _stream()),
          "umv_add_rows_bf16")
    return out


def argmax(logits, out=None):
    lib = _lib.load()
    _req(logits, BF16, "logits")
    M, V = logits.shape
    out = torch.empty((M,), dtype=torch.int64, device=logits.device) if out is None else out
    check(lib.umv_argmax_bf16(_p(logits), logits.stride(0), _p(out), M, V, _stream()), "umv_argmax_bf16")
    return out


def sample(logits, temperature, seed, step=None, out=None):
    """multinomial(softmax(logits / temperature), 1) per row (device-side counter-based RNG)."""
    lib = _lib.load()
    _req(logits, BF16, "logits")
    M, V = logits.shape
    out = torch.empty((M,), dtype=torch.int64, device=logits.device) if out is None else out
    check(lib.umv_sample_bf16(_p(logits), logits.stride(0), _p(out), M, V, float(temperature), _seed64(seed), _p(step), _stream()),
          "umv_sample_bf16")
    return out


def _row_table(rows, M, who):
    """the device pointer of a per-row sampling table (sampling.to_tensor: int64 [rows >= M, 6], contiguous, 16-byte aligned)"""
    _req(rows, torch.int64, "sample_rows")
    if not (rows.dim() == 2 and rows.shape[1] == 6 and rows.shape[0] >= M and rows.is_contiguous() and rows.data_ptr() % 16 == 0):
        raise _lib.UmvError(f"{who}: sample_rows must be a contiguous, 16-byte aligned int64 [{M}, 6] tensor (sampling.to_tensor)")
    return rows.data_ptr()


def _seed64(seed):
    """a seed as the 64-bit word the kernels key their noise with"""
    return int(seed) & (2 ** 64 - 1)


def _logits_shape(who, logits, M=None):
    """logits [>= M, V] (M = None: every row) with unit column stride -> (M, V)"""
    if logits.dim() != 2 or logits.stride(1) != 1 or (M is not None and logits.shape[0] < M):
        raise _lib.UmvError(f"{who}: logits must be [{'M' if M is None else M}, V] with unit column stride")
    return logits.shape[0] if M is None else M, logits.shape[1]


def _row_outputs(who, n, **outs):
    """the optional per-row outputs of a wrapper (name -> (tensor or None, dtype)): each a contiguous tensor of n entries"""
    for name, (t, dt) in outs.items():
        if t is not None:
            _req(t, dt, name)
            if not (t.is_contiguous() and t.numel() == n):
                raise _lib.UmvError(f"{who}: {name} must be a contiguous {dt} tensor of {n} entries")


def _tile_keys(who, M, argmax_partial=None, lse_partial=None, sample_rows=None, n_tiles=None):
    """What the lm_head epilogue leaves per 16-column tile for M rows, and the table it sampled by, checked for the wrapper `who`:
    argmax_partial int64 [M, n_tiles], lse_partial fp32 [M, n_tiles, 2], both contiguous and of one n_tiles - the caller's where it
    knows it, else the tensors' own -, and sample_rows through _row_table.  Returns the three pointers (None for what was not given)
    and n_tiles (0 without keys or statistics)."""
    amax = lse = rows = None
    if argmax_partial is not None:
        _req(argmax_partial, torch.int64, "argmax_partial")
        if not (argmax_partial.is_contiguous() and argmax_partial.dim() == 2 and argmax_partial.shape[0] == M
                and n_tiles in (None, argmax_partial.shape[1])):
            raise _lib.UmvError(f"{who}: argmax_partial must be a contiguous int64 [{M}, {'n_tiles' if n_tiles is None else n_tiles}] tensor")
        amax, n_tiles = argmax_partial.data_ptr(), argmax_partial.shape[1]
    if lse_partial is not None:
        _req(lse_partial, torch.float32, "lse_partial")
        if not (lse_partial.is_contiguous() and lse_partial.dim() == 3 and lse_partial.shape[0] == M and lse_partial.shape[2] == 2
                and n_tiles in (None, lse_partial.shape[1])):
            raise _lib.UmvError(f"{who}: lse_partial must be a contiguous fp32 [{M}, {'n_tiles' if n_tiles is None else n_tiles}, 2] tensor")
        lse, n_tiles = lse_partial.data_ptr(), lse_partial.shape[1]
    if sample_rows is not None:
        rows = _row_table(sample_rows, M, who)
    return amax, lse, rows, n_tiles or 0


def _fill_tile_keys(a, who, M, temperature, seed, step, argmax_partial, lse_partial, sample_rows):
    """the seven fields umv_logit_penalty_args and umv_logit_constrain_args share: how the lm_head call sampled, and the tiles to rewrite"""
    a.temperature, a.seed, a.step = float(temperature), _seed64(seed), None if step is None else step.data_ptr()
    a.argmax_partial, a.lse_partial, a.rows, a.n_tiles = _tile_keys(who, M, argmax_partial, lse_partial, sample_rows)


def check_truncation(top_k, top_p, min_p):
    """The filters of truncated sampling as (int, float, float), ValueError outside their ranges (0 / 1.0 / 0.0 = off)."""
    if isinstance(top_k, bool) or int(top_k) != top_k or top_k < 0:
        raise ValueError(f"top_k must be an integer >= 0 (0 = off), got {top_k!r}")
    if not 0.0 < top_p <= 1.0:
        raise ValueError(f"top_p must be in (0, 1] (1.0 = off), got {top_p!r}")
    if not 0.0 <= min_p < 1.0:
        raise ValueError(f"min_p must be in [0, 1) (0.0 = off), got {min_p!r}")
    return int(top_k), float(top_p), float(min_p)


def sample_truncated(logits, temperature, seed, step=None, top_k=0, top_p=1.0, min_p=0.0, out=None, cut_y=None, n_kept=None):
    """One draw per row from softmax(bf16(logits / temperature)) truncated by top-k / top-p / min-p (include/unimedvl_hip.h, truncated
    sampling; at least one filter on) -> int64 [M].  Same noise as the lm_head sampling epilogue for the same (seed, step, row, column).
    cut_y (fp32 [M]) / n_kept (int32 [M]), if given, receive the cutoff value and the number of kept columns."""
    lib = _lib.load()
    _req(logits, BF16, "logits")
    M, V = _logits_shape("sample_truncated", logits)
    out = torch.empty((M,), dtype=torch.int64, device=logits.device) if out is None else out
    _row_outputs("sample_truncated", M, out=(out, torch.int64), cut_y=(cut_y, torch.float32), n_kept=(n_kept, torch.int32))
    check(lib.umv_sample_truncated_bf16(_p(logits), logits.stride(0), _p(out), M, V, float(temperature), _seed64(seed), _p(step),
                                        int(top_k), float(top_p), float(min_p), _p(cut_y), _p(n_kept), _stream()),
          "umv_sample_truncated_bf16")
    return out


def check_penalties(repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, logit_bias=None, vocab=None):
    """The logit penalties (include/unimedvl_hip.h, logit penalties and bias) as (float, float, float, {int: float}), ValueError
    outside their ranges: repetition_penalty finite and > 0 (1.0 = off), presence / frequency finite (0.0 = off), logit_bias a
    {token: bias} mapping of integer tokens >= 0 (below `vocab` when given) to floats that are not NaN (-inf bans the token)."""
    import math

    def number(v, name):
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise ValueError(f"{name} must be a number, got {v!r}")
        return float(v)
    r, p, f = (number(v, n) for v, n in ((repetition_penalty, "repetition_penalty"), (presence_penalty, "presence_penalty"),
                                         (frequency_penalty, "frequency_penalty")))
    if not (math.isfinite(r) and r > 0.0):
        raise ValueError(f"repetition_penalty must be finite and > 0 (1.0 = off), got {repetition_penalty!r}")
    if not (math.isfinite(p) and math.isfinite(f)):
        raise ValueError(f"presence_penalty / frequency_penalty must be finite (0.0 = off), got {presence_penalty!r} / {frequency_penalty!r}")
    bias = {}
    if logit_bias is not None:
        if not hasattr(logit_bias, "items"):
            raise ValueError(f"logit_bias must be a {{token: bias}} mapping, got {type(logit_bias).__name__}")
        for tok, v in logit_bias.items():
            if isinstance(tok, bool) or not isinstance(tok, int) or tok < 0 or (vocab is not None and tok >= vocab):
                raise ValueError(f"logit_bias: token {tok!r} is not an integer in [0, {'vocab' if vocab is None else vocab})")
            v = number(v, f"logit_bias[{tok}]")
            if math.isnan(v):
                raise ValueError(f"logit_bias[{tok}] is NaN")
            bias[int(tok)] = v
    return r, p, f, bias


def logit_penalty(logits, ids, count, vlist, list_len, n_static, bias=None, repetition_penalty=1.0, presence_penalty=0.0,
                  frequency_penalty=0.0, temperature=0.0, seed=0, step=None, argmax_partial=None, lse_partial=None, sample_rows=None):
    """umv_logit_penalty_bf16 on bf16 logits [M, V], in place: record ids (int64 [M], the tokens this step is fed) in count (int32 [M, V])
    and the visit list vlist (int32 [M, cap], the first n_static entries seeded by the caller, bias fp32 [M, n_static] parallel to them)
    / list_len (int32 [M], -1 = fresh slot), patch the listed columns, and - with argmax_partial ([M, n_tiles] int64, lse_partial
    [M, n_tiles, 2] fp32) - recompute the tiles they sit in as the lm_head call with sample=(temperature, seed, step) leaves them
    (temperature 0: greedy).  sample_rows (the per-row table of sampling.to_tensor, int64 [M, 6]): every row takes its three penalty
    values, its temperature and its sampling key from its own entry; the scalar ones must then be left neutral."""
    lib = _lib.load()
    _req(logits, BF16, "logits")
    _req(ids, torch.int64, "ids")
    for t, name in ((count, "count"), (vlist, "list"), (list_len, "list_len")):
        _req(t, torch.int32, name)
    M, V = _logits_shape("logit_penalty", logits)
    if not (ids.is_contiguous() and ids.numel() == M and list_len.is_contiguous() and list_len.numel() == M and count.is_contiguous()
            and tuple(count.shape) == (M, V) and vlist.is_contiguous() and vlist.dim() == 2 and vlist.shape[0] == M):
        raise _lib.UmvError("logit_penalty: ids [M], count [M, V], list [M, cap], list_len [M], all contiguous")
    if bias is not None:
        _req(bias, torch.float32, "bias")
        if not (bias.is_contiguous() and tuple(bias.shape) == (M, int(n_static))):
            raise _lib.UmvError("logit_penalty: bias must be a contiguous fp32 [M, n_static] tensor")
    a = LogitPenaltyArgs()
    a.logits, a.ld, a.ids, a.count, a.list, a.list_len = logits.data_ptr(), logits.stride(0), ids.data_ptr(), count.data_ptr(), \
        vlist.data_ptr(), list_len.data_ptr()
    a.bias = None if bias is None else bias.data_ptr()
    a.M, a.V, a.cap, a.n_static = M, V, vlist.shape[1], int(n_static)
    a.repetition_penalty, a.presence_penalty, a.frequency_penalty = float(repetition_penalty), float(presence_penalty), float(frequency_penalty)
    _fill_tile_keys(a, "logit_penalty", M, temperature, seed, step, argmax_partial, lse_partial, sample_rows)
    check(lib.umv_logit_penalty_bf16(C.byref(a), _stream()), "umv_logit_penalty_bf16")
    return logits


CONSTRAIN_CHUNK = _lib.CONSTRAIN_CHUNK      # columns one workgroup of umv_logit_constrain_bf16 masks (UMV_CONSTRAIN_CHUNK)


def _automaton_args(automaton, who):
    """umv_token_automaton of a constraints.DeviceAutomaton on the current tensors' device"""
    for t, name, n in ((automaton.row_ptr, "row_ptr", automaton.n_states + 1), (automaton.edge_token, "edge_token", automaton.n_edges),
                       (automaton.edge_next, "edge_next", automaton.n_edges)):
        _req(t, torch.int32, f"automaton.{name}")
        if not (t.is_contiguous() and t.dim() == 1 and t.numel() == n):
            raise _lib.UmvError(f"{who}: automaton.{name} must be a contiguous int32 [{n}] tensor")
    t = TokenAutomatonArgs()
    t.row_ptr, t.edge_token, t.edge_next = automaton.row_ptr.data_ptr(), automaton.edge_token.data_ptr() or None, \
        automaton.edge_next.data_ptr() or None
    t.n_states, t.n_edges = int(automaton.n_states), int(automaton.n_edges)
    return t


def logit_constrain(logits, automaton, state, temperature=0.0, seed=0, step=None, argmax_partial=None, lse_partial=None, sample_rows=None):
    """umv_logit_constrain_bf16 on bf16 logits [M, V], in place: row b in state state[b] (int32 [M]) of `automaton` (a
    constraints.DeviceAutomaton) keeps the bits of the columns its state has an edge for, every other column becomes -inf; a row whose
    word is negative or >= n_states is not touched.  With argmax_partial ([M, n_tiles] int64, lse_partial [M, n_tiles, 2] fp32) every
    tile of a masked row is recomputed as the lm_head call with sample=(temperature, seed, step) leaves it for the masked logits
    (temperature 0: greedy); sample_rows (the per-row table, int64 [M, 6]): with every row's own temperature and key, the scalar
    temperature left at 0.  Runs after logit_penalty when that runs, before whatever picks."""
    lib = _lib.load()
    _req(logits, BF16, "logits")
    _req(state, torch.int32, "state")
    M, V = _logits_shape("logit_constrain", logits)
    if not (state.is_contiguous() and state.numel() == M):
        raise _lib.UmvError("logit_constrain: state must be a contiguous int32 [M] tensor")
    a = LogitConstrainArgs()
    a.logits, a.ld, a.M, a.V = logits.data_ptr(), logits.stride(0), M, V
    a.automaton = _automaton_args(automaton, "logit_constrain")
    a.state = state.data_ptr()
    _fill_tile_keys(a, "logit_constrain", M, temperature, seed, step, argmax_partial, lse_partial, sample_rows)
    check(lib.umv_logit_constrain_bf16(C.byref(a), _stream()), "umv_logit_constrain_bf16")
    return logits


def constraint_advance(automaton, state, ids):
    """umv_constraint_advance: state (int32 [M]) moves along the edge of ids (int64 [M], the tokens the step end left to be fed next) -
    to that edge's next state, to CONSTRAINT_LEFT where the row's state has no such edge; a free row keeps its word."""
    lib = _lib.load()
    _req(state, torch.int32, "state")
    _req(ids, torch.int64, "ids")
    M = state.numel()
    if not (state.is_contiguous() and ids.is_contiguous() and ids.numel() == M):
        raise _lib.UmvError("constraint_advance: state int32 [M] and ids int64 [M], both contiguous")
    t = _automaton_args(automaton, "constraint_advance")
    check(lib.umv_constraint_advance(C.byref(t), _p(state), _p(ids), M, _stream()), "umv_constraint_advance")
    return state


# what guidance_scale != 1 does not combine with, by keyword -> the value that leaves it off (beam.BEAM_EXCLUDES' precedent: refused by
# ValueError before any launch).  The later logit stages would work on the conditional row as they do today: DESIGN.md section 7.
GUIDANCE_EXCLUDES = dict(num_beams=1, draft_len=0, sampling=None, row_sampling=None, repetition_penalty=1.0, presence_penalty=0.0,
                         frequency_penalty=0.0, logit_bias=None, no_repeat_ngram_size=0, constraint=None, choices=None,
                         bad_words_ids=None, bad_words=None, suppress_tokens=None, begin_suppress_tokens=None, min_new_tokens=0,
                         forced_ids=None, return_logits=False)


def check_guidance(guidance_scale=1.0, guidance_plausibility=0.0, **kw):
    """Classifier-free guidance for text (include/unimedvl_hip.h) as (scale, beta) floats: guidance_scale finite and >= 0 (1.0 = off),
    guidance_plausibility in [0, 1) (0.0 = off), ValueError otherwise.  kw: the other keywords of the call by name (names outside
    GUIDANCE_EXCLUDES are a TypeError); with guidance on (scale != 1) one that is not off is a ValueError, and so is the unfused
    step end (UMV_DECODE_FUSED_ARGMAX=0).  guidance_plausibility without guidance is a ValueError too: there is nothing to floor."""
    import math
    import os
    unknown = set(kw) - set(GUIDANCE_EXCLUDES)
    if unknown:
        raise TypeError(f"check_guidance: unknown keywords {sorted(unknown)}")
    for v, name in ((guidance_scale, "guidance_scale"), (guidance_plausibility, "guidance_plausibility")):
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise ValueError(f"{name} must be a number, got {v!r}")
    g, beta = float(guidance_scale), float(guidance_plausibility)
    if not (math.isfinite(g) and g >= 0.0):
        raise ValueError(f"guidance_scale must be finite and >= 0 (1.0 = off), got {guidance_scale!r}")
    if not 0.0 <= beta < 1.0:
        raise ValueError(f"guidance_plausibility must be in [0, 1) (0.0 = off), got {guidance_plausibility!r}")
    if g == 1.0:
        if beta != 0.0:
            raise ValueError("guidance_plausibility floors the guided distribution: it needs guidance_scale != 1")
        return g, beta

    def off(value, neutral):
        if isinstance(value, (list, tuple)):
            return all(off(v, neutral) for v in value) if neutral is not None or len(value) == 0 else False
        if neutral is None:
            return value is None or value == {}
        return value == neutral
    on = [k for k, v in kw.items() if not off(v, GUIDANCE_EXCLUDES[k])]
    if on:
        raise ValueError(f"guidance_scale != 1 (classifier-free guidance for text) excludes {', '.join(sorted(on))}")
    if os.environ.get("UMV_DECODE_FUSED_ARGMAX", "1") in ("0", ""):
        raise ValueError("guidance_scale != 1 rides on the fused step end: UMV_DECODE_FUSED_ARGMAX must not be 0")
    return g, beta


def check_guidance_pairs(pair, rows=None):
    """A pair table (include/unimedvl_hip.h: pair[c] = the unconditional row of guided row c, -1 = not guided) as a list of ints,
    ValueError for what the kernels would only ignore: an entry outside [-1, rows), a row paired with itself, a row that is both
    guided and someone's unconditional row, two guided rows that share one."""
    pair = [int(v) for v in (pair.tolist() if hasattr(pair, "tolist") else pair)]
    rows = len(pair) if rows is None else int(rows)
    if len(pair) != rows:
        raise ValueError(f"the pair table must hold one entry per row ({rows}), got {len(pair)}")
    taken = {}
    for c, u in enumerate(pair):
        if u == -1:
            continue
        if not 0 <= u < rows or u == c:
            raise ValueError(f"pair[{c}] = {u}: an unconditional row is another row of [0, {rows}), or -1")
        if u in taken:
            raise ValueError(f"rows {taken[u]} and {c} share the unconditional row {u}")
        taken[u] = c
    for c, u in enumerate(pair):
        if u != -1 and c in taken:
            raise ValueError(f"row {c} is guided (by row {u}) and the unconditional row of row {taken[c]}")
    return pair


def logit_guidance(logits, pair, scale, log_beta, lse, row_max, stats=None, temperature=0.0, seed=0, step=None, argmax_partial=None,
                   lse_partial=None):
    """umv_logit_guidance_bf16 on bf16 logits [M, V], in place: every active row c (pair int32 [M], scale / log_beta fp32 [M]) becomes
    bf16(scale[c] * (log_softmax(l_c) - log_softmax(l_u)) + log_softmax(l_u)), u = pair[c], under the plausibility floor log_beta[c]
    (include/unimedvl_hip.h, classifier-free guidance for text); lse / row_max (fp32 [M]) receive the log-sum-exp and the maximum of
    the rows that took part.  With argmax_partial ([M, n_tiles] int64, lse_partial [M, n_tiles, 2] fp32) every tile of a rewritten row
    is recomputed as the lm_head call with sample=(temperature, seed, step) leaves it.  stats (fp32 [M, n_tiles, 2]): the workspace of
    the temperature-0 tile pairs, needed unless lse_partial holds them (temperature 0 or 1).  Runs first behind the lm_head call."""
    lib = _lib.load()
    _req(logits, BF16, "logits")
    M, V = _logits_shape("logit_guidance", logits)
    _req(pair, torch.int32, "pair")
    if not (pair.is_contiguous() and pair.numel() == M):
        raise _lib.UmvError("logit_guidance: pair must be a contiguous int32 [M] tensor")
    _row_outputs("logit_guidance", M, scale=(scale, torch.float32), log_beta=(log_beta, torch.float32), lse=(lse, torch.float32),
                 row_max=(row_max, torch.float32))
    n_tiles = (V + 15) // 16
    if stats is not None:
        _req(stats, torch.float32, "stats")
        if not (stats.is_contiguous() and tuple(stats.shape) == (M, n_tiles, 2)):
            raise _lib.UmvError(f"logit_guidance: stats must be a contiguous fp32 [{M}, {n_tiles}, 2] tensor")
    a = _lib.LogitGuidanceArgs()
    a.logits, a.ld, a.M, a.V = logits.data_ptr(), logits.stride(0), M, V
    a.pair, a.scale, a.log_beta, a.lse, a.row_max = (None if t is None else t.data_ptr() for t in (pair, scale, log_beta, lse, row_max))
    a.stats = None if stats is None else stats.data_ptr()
    a.temperature, a.seed, a.step = float(temperature), _seed64(seed), None if step is None else step.data_ptr()
    a.argmax_partial, a.lse_partial, _, _ = _tile_keys("logit_guidance", M, argmax_partial, lse_partial, None, n_tiles=n_tiles)
    a.n_tiles = n_tiles
    check(lib.umv_logit_guidance_bf16(C.byref(a), _stream()), "umv_logit_guidance_bf16")
    return logits


def guidance_feed(pair, ids, in_ids, pred_ids, step_idx):
    """umv_guidance_feed, behind the step end: for every guided row c (pair int32 [M]) the token the step end left for c - ids[c] and
    this step's pred_ids / in_ids words ([max_len, M] int64) - is copied into the words of its unconditional row pair[c]; step_idx
    (int64 [M]) as the step end left it."""
    lib = _lib.load()
    _req(pair, torch.int32, "pair")
    for t, name in ((ids, "ids"), (in_ids, "in_ids"), (pred_ids, "pred_ids"), (step_idx, "step_idx")):
        _req(t, torch.int64, name)
    M = pair.numel()
    if not (pair.is_contiguous() and ids.is_contiguous() and ids.numel() == M and step_idx.is_contiguous() and step_idx.numel() >= M
            and in_ids.is_contiguous() and pred_ids.is_contiguous() and in_ids.dim() == 2 and in_ids.shape == pred_ids.shape
            and in_ids.shape[1] == M):
        raise _lib.UmvError("guidance_feed: pair int32 [M], ids / step_idx int64 [M], in_ids / pred_ids int64 [max_len, M], all contiguous")
    check(lib.umv_guidance_feed(_p(pair), _p(ids), _p(in_ids), _p(pred_ids), _p(step_idx), M, in_ids.shape[0], _stream()),
          "umv_guidance_feed")
    return ids


NGRAM_MAX = _lib.NGRAM_MAX      # the largest no_repeat_ngram_size (UMV_NGRAM_MAX)


def check_ngram(n, what="no_repeat_ngram_size"):
    """A no_repeat_ngram_size (include/unimedvl_hip.h, no-repeat n-grams) as an int, ValueError unless it is an integer in
    [0, NGRAM_MAX] (0 = off)."""
    if isinstance(n, bool) or not isinstance(n, (int, float)) or not 0 <= n <= NGRAM_MAX or int(n) != n:
        raise ValueError(f"{what} must be an integer in [0, {NGRAM_MAX}] (0 = off), got {n!r}")
    return int(n)


def logit_ngram_ban(logits, ids, hist, hist_len, n=0, row_n=None, temperature=0.0, seed=0, step=None, argmax_partial=None,
                    lse_partial=None, sample_rows=None):
    """umv_logit_ngram_ban_bf16 on bf16 logits [M, V], in place: append ids (int64 [M], the tokens this step is fed) to the rows'
    histories (hist int32 [M, hist_ld], hist_len int32 [M]: negative = the row is off) and set to -inf every column that would repeat
    an n-gram of the row's history - n the scalar size, or row_n (int32 [M]) one per row; a size outside 1..NGRAM_MAX records only.
    With argmax_partial ([M, n_tiles] int64, lse_partial [M, n_tiles, 2] fp32) the tiles of the banned columns are recomputed as the
    lm_head call with sample=(temperature, seed, step) leaves them (temperature 0: greedy); sample_rows (the per-row table, int64
    [M, 6]): with every row's own temperature and key, the scalar temperature left at 0.  Runs after logit_penalty and before
    logit_constrain when those run, before whatever picks."""
    lib = _lib.load()
    _req(logits, BF16, "logits")
    _req(ids, torch.int64, "ids")
    _req(hist, torch.int32, "hist")
    _req(hist_len, torch.int32, "hist_len")
    M, V = _logits_shape("logit_ngram_ban", logits)
    if not (ids.is_contiguous() and ids.numel() == M and hist_len.is_contiguous() and hist_len.numel() == M and hist.is_contiguous()
            and hist.dim() == 2 and hist.shape[0] == M):
        raise _lib.UmvError("logit_ngram_ban: ids [M], hist [M, hist_ld], hist_len [M], all contiguous")
    if row_n is not None:
        _req(row_n, torch.int32, "row_n")
        if not (row_n.is_contiguous() and row_n.numel() == M):
            raise _lib.UmvError("logit_ngram_ban: row_n must be a contiguous int32 [M] tensor")
    a = NgramBanArgs()
    a.logits, a.ld, a.ids = logits.data_ptr(), logits.stride(0), ids.data_ptr()
    a.hist, a.hist_ld, a.hist_len = hist.data_ptr() or None, hist.shape[1], hist_len.data_ptr()
    a.row_n = None if row_n is None else row_n.data_ptr()
    a.M, a.V, a.n = M, V, int(n)
    _fill_tile_keys(a, "logit_ngram_ban", M, temperature, seed, step, argmax_partial, lse_partial, sample_rows)
    check(lib.umv_logit_ngram_ban_bf16(C.byref(a), _stream()), "umv_logit_ngram_ban_bf16")
    return logits


# ----------------------------------------------------------------------------- banned sequences (include/unimedvl_hip.h)
SEQ_MAX, SEQ_ENTRIES_MAX, SEQ_ROW = _lib.SEQ_MAX, _lib.SEQ_ENTRIES_MAX, _lib.SEQ_ROW
SEQ_TAIL = SEQ_MAX - 1          # history words a row keeps: what the longest entry compares


def _token_list(tokens, what, vocab):
    """a list of token ids as ints, each in [0, vocab) (vocab None: below 2^31); ValueError otherwise"""
    if tokens is None:
        return []
    if hasattr(tokens, "tolist"):
        tokens = tokens.tolist()
    if isinstance(tokens, (str, bytes)) or not isinstance(tokens, (list, tuple)):
        raise ValueError(f"{what} must be a list of token ids, got {tokens!r}")
    top = (1 << 31) if vocab is None else int(vocab)
    out = []
    for t in tokens:
        if isinstance(t, bool) or not isinstance(t, (int, float)) or int(t) != t or not 0 <= t < top:
            raise ValueError(f"{what} holds {t!r}: a token id is an integer in [0, {top})")
        out.append(int(t))
    return out


def check_sequences(bad_words_ids=None, suppress_tokens=None, begin_suppress_tokens=None, min_new_tokens=0, end_token_id=None,
                    vocab=None, rows=None):
    """The banned-sequence keywords checked and normalised: (bad_words_ids as a list of int lists, suppress_tokens and
    begin_suppress_tokens as int lists, min_new_tokens as an int - or, where a list of one per sample (`rows` of them) was given, as a
    list of ints -, end_token_id as an int or None).  ValueError: a bad word that is no non-empty list of at most SEQ_MAX token ids,
    a token outside [0, vocab), a negative or fractional min_new_tokens, min_new_tokens > 0 without end_token_id, more than
    SEQ_ENTRIES_MAX entries in all."""
    if bad_words_ids is None:
        bad_words_ids = []
    if hasattr(bad_words_ids, "tolist"):
        bad_words_ids = bad_words_ids.tolist()
    if isinstance(bad_words_ids, (str, bytes)) or not isinstance(bad_words_ids, (list, tuple)):
        raise ValueError(f"bad_words_ids must be a list of token id lists, got {bad_words_ids!r}")
    words = []
    for w in bad_words_ids:
        if isinstance(w, (int, float)):
            raise ValueError(f"bad_words_ids must be a list of token id LISTS, got the entry {w!r}")
        w = _token_list(w, "a bad_words_ids entry", vocab)
        if not 1 <= len(w) <= SEQ_MAX:
            raise ValueError(f"a bad_words_ids entry holds 1 to {SEQ_MAX} tokens, got {len(w)}")
        words.append(w)
    suppress = _token_list(suppress_tokens, "suppress_tokens", vocab)
    begin = _token_list(begin_suppress_tokens, "begin_suppress_tokens", vocab)

    def one_min(n):
        if isinstance(n, bool) or not isinstance(n, (int, float)) or int(n) != n or not 0 <= n < (1 << 31):
            raise ValueError(f"min_new_tokens must be a non-negative integer (0 = off), got {n!r}")
        return int(n)
    if min_new_tokens is None:
        min_new_tokens = 0
    if hasattr(min_new_tokens, "tolist"):
        min_new_tokens = min_new_tokens.tolist()
    if isinstance(min_new_tokens, (list, tuple)):
        mins = [one_min(n) for n in min_new_tokens]
        if rows is not None and len(mins) != rows:
            raise ValueError(f"min_new_tokens must be one integer or one per sample ({rows}), got {len(mins)}")
        any_min = any(mins)
    else:
        mins = one_min(min_new_tokens)
        any_min = mins > 0
    end = None
    if end_token_id is not None:
        end = _token_list([end_token_id], "end_token_id", vocab)[0]
    if any_min and end is None:
        raise ValueError("min_new_tokens needs end_token_id: it is the end token that is banned")
    if len(words) + len(suppress) + len(begin) + bool(any_min) > SEQ_ENTRIES_MAX:
        raise ValueError(f"at most {SEQ_ENTRIES_MAX} banned sequences and suppressed tokens in all (min_new_tokens takes one), got "
                         f"{len(words) + len(suppress) + len(begin) + bool(any_min)}")
    return words, suppress, begin, mins, end


def sequence_table(bad_words_ids=None, suppress_tokens=None, begin_suppress_tokens=None, min_new_tokens=0, end_token_id=None,
                   vocab=None, row_entry=False):
    """The CSR table of the banned-sequence stage from HF's keywords: (seq_ptr int32 [S + 1], seq_tok int32 [n_tok], seq_until int32
    [S], max_m) as numpy arrays and an int - entries (w, 0) for every bad word, ([t], 0) for every suppressed token, ([t], 1) for every
    token suppressed at the beginning and, where min_new_tokens is on for any sample (or row_entry asks for it: rows that come later
    bring their own minimum), ([end_token_id], SEQ_ROW).  S = 0 (max_m 0) when everything is off."""
    import numpy as np
    words, suppress, begin, mins, end = check_sequences(bad_words_ids, suppress_tokens, begin_suppress_tokens, min_new_tokens, end_token_id,
                                                        vocab)
    entries = [(w, 0) for w in words] + [([t], 0) for t in suppress] + [([t], 1) for t in begin]
    if (any(mins) if isinstance(mins, list) else mins > 0) or (row_entry and end is not None):
        entries.append(([end], SEQ_ROW))
    ptr, tok = [0], []
    for w, _ in entries:
        tok += w
        ptr.append(len(tok))
    return (np.array(ptr, dtype=np.int32), np.array(tok, dtype=np.int32), np.array([u for _, u in entries], dtype=np.int32),
            max([len(w) for w, _ in entries] + [0]))


def encode_bad_words(tokenizer, bad_words):
    """bad_words (strings) as bad_words_ids: every string encoded bare and with a leading space - inside a sentence a word follows a
    space, and most tokenizers give that another first token - both kept, duplicates and empty encodings dropped.  ValueError for
    what is no list of non-empty strings."""
    if bad_words is None:
        return []
    if isinstance(bad_words, str) or not isinstance(bad_words, (list, tuple)):
        raise ValueError(f"bad_words must be a list of strings, got {bad_words!r}")
    out = []
    for w in bad_words:
        if not isinstance(w, str) or not w.strip():
            raise ValueError(f"bad_words holds {w!r}: a bad word is a non-empty string")
        for text in (w, " " + w):
            ids = [int(t) for t in tokenizer.encode(text)]
            if ids and ids not in out:
                out.append(ids)
    return out


class SequenceTable:
    """A banned-sequence table in device memory (umv_sequence_ban_args: seq_ptr / seq_tok / seq_until, S, n_tok, max_m).  The entry
    lengths and offsets are validated here, on the host: the kernel entry cannot read them."""

    def __init__(self, seq_ptr, seq_tok, seq_until, device, max_m=None):
        import numpy as np
        ptr, tok, until = (np.asarray(v, dtype=np.int64).reshape(-1) for v in (seq_ptr, seq_tok, seq_until))
        S = until.size
        if not 0 <= S <= SEQ_ENTRIES_MAX or ptr.size != S + 1 or ptr[0] != 0 or ptr[-1] != tok.size:
            raise ValueError(f"a sequence table holds 0 to {SEQ_ENTRIES_MAX} entries, seq_ptr [S + 1] from 0 to len(seq_tok)")
        lens = np.diff(ptr)
        if S and (lens.min() < 1 or lens.max() > SEQ_MAX):
            raise ValueError(f"a sequence table entry holds 1 to {SEQ_MAX} tokens")
        if S and (until.min() < SEQ_ROW or until.max() >= 1 << 31 or np.abs(tok).max() >= 1 << 31):
            raise ValueError("a sequence table's until words are SEQ_ROW, 0 or a positive int32; its tokens are int32")
        longest = int(lens.max()) if S else 0
        if max_m is not None and int(max_m) != longest:
            raise ValueError(f"max_m = {max_m}, the longest entry holds {longest} tokens")
        self.S, self.n_tok, self.max_m = S, int(tok.size), longest
        self.ptr = torch.tensor(ptr.tolist(), dtype=torch.int32).to(device)
        self.tok = torch.tensor(tok.tolist() or [0], dtype=torch.int32).to(device)
        self.until = torch.tensor(until.tolist() or [0], dtype=torch.int32).to(device)


def logit_sequence_ban(logits, ids, table, tail=None, count=None, row_min=None, beam=None, temperature=0.0, seed=0, step=None,
                       argmax_partial=None, lse_partial=None, sample_rows=None):
    """umv_logit_sequence_ban_bf16 on bf16 logits [M, V], in place, against `table` (a SequenceTable).  Plain form: record ids (int64
    [M], the tokens this step is fed) in tail (int32 [M, SEQ_TAIL]) and count (int32 [M]: negative = the row is off), then set to -inf
    the last token's column of every entry that is active for the row's count - row_min (int32 [M], optional) for SEQ_ROW entries -
    and whose first tokens are the row's last.  Beam form: beam = (beam_tok, beam_parent, step_idx, start_ids, K), the back-pointers
    (int32 [max_len, M]) and row counters (int64 [M]) of a beam search and one start token per request (int64 [M / K]); nothing is
    recorded.  With argmax_partial ([M, n_tiles] int64, lse_partial [M, n_tiles, 2] fp32) the banned columns' tiles are recomputed as
    the lm_head call with sample=(temperature, seed, step) leaves them; sample_rows: with every row's own temperature and key.  Runs
    after logit_penalty and logit_ngram_ban and before logit_constrain when those run, before whatever picks."""
    lib = _lib.load()
    _req(logits, BF16, "logits")
    _req(ids, torch.int64, "ids")
    M, V = _logits_shape("logit_sequence_ban", logits)
    if not isinstance(table, SequenceTable):
        raise _lib.UmvError("logit_sequence_ban: table must be an ops.SequenceTable")
    if not (ids.is_contiguous() and ids.numel() == M):
        raise _lib.UmvError("logit_sequence_ban: ids must be a contiguous int64 [M] tensor")
    a = _lib.SequenceBanArgs()
    a.logits, a.ld, a.ids = logits.data_ptr(), logits.stride(0), ids.data_ptr()
    if table.S:
        a.seq_ptr, a.seq_tok, a.seq_until = table.ptr.data_ptr(), table.tok.data_ptr(), table.until.data_ptr()
    a.M, a.V, a.S, a.n_tok, a.max_m = M, V, table.S, table.n_tok, table.max_m
    if row_min is not None:
        _row_outputs("logit_sequence_ban", M, row_min=(row_min, torch.int32))
        a.row_min = row_min.data_ptr()
    if beam is None:
        if tail is None or count is None:
            raise _lib.UmvError("logit_sequence_ban: the plain form needs tail and count")
        _req(tail, torch.int32, "tail")
        _req(count, torch.int32, "count")
        if not (tail.is_contiguous() and tuple(tail.shape) == (M, SEQ_TAIL) and count.is_contiguous() and count.numel() == M):
            raise _lib.UmvError(f"logit_sequence_ban: tail [M, {SEQ_TAIL}] and count [M], both contiguous")
        a.tail, a.count = tail.data_ptr() or None, count.data_ptr() or None
    else:
        beam_tok, beam_parent, step_idx, start_ids, K = beam
        K = int(K)
        if tail is not None or count is not None:
            raise _lib.UmvError("logit_sequence_ban: the beam form keeps no tail / count")
        if not 1 <= K <= _lib.BEAM_K_MAX or M % K:
            raise _lib.UmvError(f"logit_sequence_ban: K = {K} must be in [1, {_lib.BEAM_K_MAX}] and divide M = {M}")
        _req(beam_tok, torch.int32, "beam_tok")
        _req(beam_parent, torch.int32, "beam_parent")
        if not (beam_tok.is_contiguous() and beam_tok.dim() == 2 and beam_tok.shape[1] == M and beam_tok.shape[0] >= 1
                and beam_parent.is_contiguous() and beam_parent.shape == beam_tok.shape):
            raise _lib.UmvError("logit_sequence_ban: beam_tok / beam_parent must be contiguous int32 [max_len, M] tensors of one shape")
        _row_outputs("logit_sequence_ban", M, step_idx=(step_idx, torch.int64))
        _row_outputs("logit_sequence_ban", M // K, start_ids=(start_ids, torch.int64))
        a.beam_tok, a.beam_parent, a.step_idx, a.start_ids = (t.data_ptr() for t in (beam_tok, beam_parent, step_idx, start_ids))
        a.K, a.max_len = K, beam_tok.shape[0]
    _fill_tile_keys(a, "logit_sequence_ban", M, temperature, seed, step, argmax_partial, lse_partial, sample_rows)
    check(lib.umv_logit_sequence_ban_bf16(C.byref(a), _stream()), "umv_logit_sequence_ban_bf16")
    return logits


def cast_pad(x, Kp):
    lib = _lib.load()
    _req(x, torch.float32, "x")
    T, K = x.shape
    out = torch.empty((T, Kp), dtype=BF16, device=x.device)
    check(lib.umv_cast_pad_f32_bf16(_p(x), x.stride(0), _p(out), Kp, T, K, Kp, _stream()), "umv_cast_pad_f32_bf16")
    return out


def patchify(img, out, patch):
    """Transformed image [C, H, W] fp32 (device) -> its patch tokens, cast to bf16 and zero padded, into out [(H/p)*(W/p), Kp]."""
    lib = _lib.load()
    _req(img, torch.float32, "img")
    _req(out, BF16, "out")
    if img.dim() != 3 or not img.is_contiguous() or out.dim() != 2 or out.stride(1) != 1:
        raise _lib.UmvError("patchify: img must be a contiguous [C, H, W] tensor, out a [tokens, Kp] view with unit column stride")
    C_, H, W = img.shape
    if out.shape[0] != (H // patch) * (W // patch):
        raise _lib.UmvError(f"patchify: out has {out.shape[0]} rows, the image has {(H // patch) * (W // patch)} patches")
    check(lib.umv_patchify_f32_bf16(_p(img), C_, H, W, patch, _p(out), out.stride(0), out.shape[1], _stream()), "umv_patchify_f32_bf16")
    return out


class KVSlab:
    """One layer's K / V^T slabs: K [seg][nkv][cap][hd], V^T [seg][nkv][hd][cap]."""

    __slots__ = ("k", "vt", "nseg", "nkv", "cap", "hd")

    def __init__(self, nseg, nkv, cap, hd, device, keys=True):
        """keys=False: V^T only - K is read in place from a packed buffer (attention(..., k_packed=...))."""
        assert cap % 32 == 0
        self.k = torch.zeros((nseg, nkv, cap, hd), dtype=BF16, device=device) if keys else None
        self.vt = torch.zeros((nseg, nkv, hd, cap), dtype=BF16, device=device)
        self.nseg, self.nkv, self.cap, self.hd = nseg, nkv, cap, hd

    @staticmethod
    def from_tensors(k, vt):
        """Wrap existing (possibly sliced along the segment dim) slab tensors."""
        s = KVSlab.__new__(KVSlab)
        s.k, s.vt = k, vt
        s.nseg, s.nkv, s.cap, s.hd = k.shape
        assert k.stride(3) == 1 and k.stride(2) == s.hd and k.stride(1) == s.cap * s.hd and k.stride(0) == s.nkv * s.cap * s.hd
        return s

    def strides(self):
        return dict(k_seg_stride=self.nkv * self.cap * self.hd, k_head_stride=self.cap * self.hd,
                    v_seg_stride=self.nkv * self.hd * self.cap, v_head_stride=self.hd * self.cap, v_d_stride=self.cap)


KV_PAGE = 256      # keys per page of a paged KV pool (UMV_KV_PAGE)


class PagedSlab:
    """One layer's K / V^T page POOLS of a paged cache (kvcache.PagedCache): K [page][nkv][256][hd], V^T [page][nkv][hd][256], shared
    by all segments through `table` ([nseg, max_pages] int32 on the device: entry p of segment s = the pool page of its keys p*256 ..).
    Stands in for a KVSlab in qkv_post() / attention(): same strides() contract with "segment" read as "page"."""

    __slots__ = ("k", "vt", "table", "nkv", "hd", "cap")

    def __init__(self, npages, nkv, hd, device, table):
        self.k = torch.zeros((npages, nkv, KV_PAGE, hd), dtype=BF16, device=device)
        self.vt = torch.zeros((npages, nkv, hd, KV_PAGE), dtype=BF16, device=device)
        self.table, self.nkv, self.hd = table, nkv, hd
        self.cap = table.shape[1] * KV_PAGE          # longest context the table can describe

    def strides(self):
        return dict(k_seg_stride=self.nkv * KV_PAGE * self.hd, k_head_stride=KV_PAGE * self.hd,
                    v_seg_stride=self.nkv * self.hd * KV_PAGE, v_head_stride=self.hd * KV_PAGE, v_d_stride=KV_PAGE)


def _paging(slab):
    t = getattr(slab, "table", None)
    return {} if t is None else dict(page_table=t.data_ptr(), page_table_stride=t.stride(0))


def quantize_act(x, M=None, row_idx=None, K=None):
    """Per-row e4m3 quantisation of bf16 activations (umv_quantize_act_fp8): returns (xq uint8 [M, ldq], scale f32 [M]).
    K: the columns that count (a linear's K) when x is wider"""
    lib = _lib.load()
    _req(x, BF16, "x")
    M = x.shape[0] if M is None else M
    K = x.shape[1] if K is None else K
    ldq = (K + 127) // 128 * 128
    xq = torch.empty((M, ldq), dtype=torch.uint8, device=x.device)
    xs = torch.empty((M,), dtype=torch.float32, device=x.device)
    check(lib.umv_quantize_act_fp8(_p(x), x.stride(0), _p(row_idx), _p(xq), ldq, _p(xs), None, 0, M, K, _stream()), "umv_quantize_act_fp8")
    return xq, xs


def fake_quantize_act(x, M=None, row_idx=None):
    """bf16 copy of x whose rows (row_idx[m] when given, the others are left undefined) are rounded through the per-row e4m3
    grid: the activations of the W8A8 mode for the M <= 64 kernels, which take bf16 inputs."""
    lib = _lib.load()
    _req(x, BF16, "x")
    M = x.shape[0] if M is None else M
    out = torch.empty_like(x)
    xs = torch.empty((M,), dtype=torch.float32, device=x.device)
    ldq = (x.shape[1] + 127) // 128 * 128
    check(lib.umv_quantize_act_fp8(_p(x), x.stride(0), _p(row_idx), None, ldq, _p(xs), _p(out), out.stride(0), M, x.shape[1], _stream()),
          "umv_quantize_act_fp8")
    return out


def _sample_fields(sample, amax):
    """(sample_temperature, sample_seed, sample_step) of gemm's sample=(temperature, seed, step tensor or None)"""
    if amax is None:
        raise _lib.UmvError("gemm: sample=(temperature, seed, step) is a mode of the argmax_partial epilogue")
    t, seed, step = sample
    if not float(t) > 0.0:
        raise _lib.UmvError(f"gemm: sampling temperature must be > 0 (got {t})")
    return float(t), _seed64(seed), None if step is None else step.data_ptr()


def gemm_splitk(x, lin, partials, k_splits, *, M=None, z13=None):
    """Split-K decode GEMM (M <= 64): raw fp32 partial sums [k_splits, rows, N] into `partials`; the consumer
    (qkv_post(partials=...) / residual_rmsnorm) adds the splits and finishes the row.  z13: as in gemm (tests and A/B only)."""
    lib = _lib.load()
    _req(x, BF16, "x")
    _req(partials, torch.float32, "partials")
    M = x.shape[0] if M is None else M
    assert partials.dim() == 3 and partials.shape[0] == k_splits and partials.shape[2] == lin.N and partials.is_contiguous()
    assert lin.th == 16 and not lin.swiglu
    route = _route(lin, M, True, z13=z13)
    return _launch(lib, route, x, lin, partials, lin.N, M, k_splits=k_splits, split_stride=partials.stride(0))


def residual_rmsnorm(partials, seq, w, eps, out):
    """seq = bf16(bf16(sum_s partials[s]) + seq) in place; out = RMSNorm(seq) * w.  partials [S, T, H] fp32."""
    lib = _lib.load()
    _req(partials, torch.float32, "partials")
    _req(seq, BF16, "seq")
    S, T, H = partials.shape
    assert seq.shape == (T, H) and seq.is_contiguous() and out.is_contiguous() and partials.is_contiguous()
    check(lib.umv_residual_rmsnorm_bf16(_p(partials), S, partials.stride(0), partials.stride(1), _p(seq), _p(w), _p(out), T, H, eps,
                                        _stream()), "umv_residual_rmsnorm_bf16")
    return out


def qkv_post(qkv, q_out, slab, tok_seg, tok_slot, tok_pos, nq, nkv, hd, eps=1e-6, q_norm=None, k_norm=None,
             q_norm_gen=None, k_norm_gen=None, expert=None, cos_tab=None, sin_tab=None, T=None, fp32_chain=False,
             partials=None, bias=None):
    """partials (fp32 [S, T, (nq+2nkv)*hd]) + bias: take the QKV row from a split-K GEMM instead of `qkv`.
    q_out=None with a keys=False slab: only V is split off (into V^T); q and K are then read in place by attention()."""
    if (q_out is None) != (slab.k is None):
        raise _lib.UmvError("qkv_post: q_out=None (V-only split) goes with a KVSlab(keys=False), and only with it")
    lib = _lib.load()
    if partials is None:
        _req(qkv, BF16, "qkv")
        T = qkv.shape[0] if T is None else T
    else:
        _req(partials, torch.float32, "partials")
        T = partials.shape[1] if T is None else T
    a = QkvPostArgs(
        qkv=None if qkv is None else qkv.data_ptr(),
        qkv_partials=None if partials is None else partials.data_ptr(),
        n_splits=0 if partials is None else partials.shape[0],
        split_stride=0 if partials is None else partials.stride(0),
        qkv_bias=None if bias is None else bias.data_ptr(),
        q_out=None if q_out is None else q_out.data_ptr(), k_slab=None if slab.k is None else slab.k.data_ptr(), vt_slab=slab.vt.data_ptr(),
        tok_seg=tok_seg.data_ptr(), tok_slot=tok_slot.data_ptr(),
        tok_pos=None if tok_pos is None else tok_pos.data_ptr(),
        expert=None if expert is None else expert.data_ptr(),
        q_norm_w=None if q_norm is None else q_norm.data_ptr(), k_norm_w=None if k_norm is None else k_norm.data_ptr(),
        q_norm_w_gen=None if q_norm_gen is None else q_norm_gen.data_ptr(),
        k_norm_w_gen=None if k_norm_gen is None else k_norm_gen.data_ptr(),
        cos_tab=None if cos_tab is None else cos_tab.data_ptr(), sin_tab=None if sin_tab is None else sin_tab.data_ptr(),
        T=T, nq=nq, nkv=nkv, hd=hd, eps=eps, fp32_chain=int(fp32_chain), **slab.strides(), **_paging(slab))
    check(lib.umv_qkv_post(C.byref(a), _stream()), "umv_qkv_post")


def attn_workspace(nseg, nq, hd, max_q, nsplit, device):
    n = _lib.load().umv_attn_workspace_bytes(nseg, nq, hd, max_q, nsplit)
    return torch.empty(max(n, 16) // 4, dtype=torch.float32, device=device)


def attention(q, out, slab, cu_q, kv_len, nq, nkv, hd, causal, max_q, max_kv, nsplit=1, workspace=None, k_packed=None,
              _entry=None, variant=0, stats=None, wave_split=0):
    """q: [T, nq*hd] or [T, nq, hd] rows, possibly a column slice of a wider buffer (row stride = q.stride(0)).
    k_packed: [T, nkv*hd] column slice holding K row-aligned with q (cache-less self-attention): the K slab is not read.
    _entry: (function, checker, name) of another library taking the same umv_attn_args (experimental/ops.py; tests / tools only).
    variant / stats: umv_attn_args.variant (_lib.ATTN_* bits) and the two uint32 rare-path counters (tests / A-B only)."""
    lib = _lib.load()
    _req(q, BF16, "q")
    if q.stride(-1) != 1 or (q.dim() == 3 and q.stride(1) != hd):
        raise _lib.UmvError("attention: q rows must be contiguous [nq * hd] runs")
    strides = slab.strides()
    if k_packed is not None:
        _req(k_packed, BF16, "k_packed")
        if k_packed.dim() != 2 or k_packed.stride(1) != 1 or k_packed.shape[0] != q.shape[0] or k_packed.shape[1] != nkv * hd:
            raise _lib.UmvError("attention: k_packed must be a [T, nkv*hd] view with unit column stride")
        k_ptr, k_key_stride = k_packed.data_ptr(), k_packed.stride(0)
        strides["k_head_stride"] = hd
    else:
        if slab.k is None:
            raise _lib.UmvError("attention: this KVSlab holds no keys (keys=False) - pass k_packed")
        k_ptr, k_key_stride = slab.k.data_ptr(), 0
    a = AttnArgs(
        q=q.data_ptr(), out=out.data_ptr(), cu_q=cu_q.data_ptr(), kv_len=kv_len.data_ptr(),
        k_slab=k_ptr, vt_slab=slab.vt.data_ptr(), nseg=kv_len.numel(), nq=nq, nkv=nkv, hd=hd,
        causal=int(bool(causal)), max_q=max_q, max_kv=max_kv, nsplit=nsplit,
        workspace=None if workspace is None else workspace.data_ptr(), q_row_stride=q.stride(0), k_key_stride=k_key_stride,
        variant=int(variant), stats=None if stats is None else stats.data_ptr(), wave_split=int(wave_split), **strides, **_paging(slab))
    if _entry is not None:
        fn, chk, name = _entry
        chk(fn(C.byref(a), _stream()), name)
        return out
    check(lib.umv_attn_varlen(C.byref(a), _stream()), "umv_attn_varlen")
    return out


def decode_advance(tok_slot, tok_pos, kv_len):
    lib = _lib.load()
    check(lib.umv_decode_advance(_p(tok_slot), _p(tok_pos), _p(kv_len), tok_slot.numel(), _stream()), "umv_decode_advance")


def decode_step_end(tok_slot, tok_pos, kv_len, ids, in_ids, pred_ids, step_idx):
    """pred_ids[s] = ids, in_ids[s + 1] = ids, counters += 1, s += 1 - the whole bookkeeping of a decode step in one launch."""
    lib = _lib.load()
    for t, name in ((ids, "ids"), (in_ids, "in_ids"), (pred_ids, "pred_ids"), (step_idx, "step_idx")):
        _req(t, torch.int64, name)
    if not (in_ids.is_contiguous() and pred_ids.is_contiguous() and in_ids.shape == pred_ids.shape and in_ids.shape[1] == ids.numel()):
        raise _lib.UmvError("decode_step_end: in_ids / pred_ids must be contiguous [max_len, B]")
    check(lib.umv_decode_step_end(_p(tok_slot), _p(tok_pos), _p(kv_len), _p(ids), _p(in_ids), _p(pred_ids), _p(step_idx),
                                  ids.numel(), in_ids.shape[0], _stream()), "umv_decode_step_end")


def _check_fused_step_end(who, argmax_partial, ids, in_ids, pred_ids, step_idx, lse_partial=None, logits=None, **rows):
    """What the decode_step_end_* wrappers below check alike, under the wrapper's name: int64 keys / ids / counters, one counter per sample,
    contiguous in_ids / pred_ids [max_len, B] and argmax_partial [B, n_tiles], lse_partial [B, n_tiles, 2] where there is one, the
    optional [max_len, B] tensors in `rows` (name -> (tensor or None, dtype)) and bf16 logits [B, V].  Returns B."""
    for t, name in ((ids, "ids"), (in_ids, "in_ids"), (pred_ids, "pred_ids"), (step_idx, "step_idx")):
        _req(t, torch.int64, name)
    B = ids.numel()
    if step_idx.numel() < B:
        raise _lib.UmvError(f"{who}: step_idx holds {step_idx.numel()} counters for {B} samples")
    if not (in_ids.is_contiguous() and pred_ids.is_contiguous() and in_ids.shape == pred_ids.shape and in_ids.shape[1] == B):
        raise _lib.UmvError(f"{who}: in_ids / pred_ids must be contiguous [max_len, B]")
    _tile_keys(who, B, _req(argmax_partial, torch.int64, "argmax_partial"), lse_partial)
    for name, (t, dt) in rows.items():
        if t is not None:
            _req(t, dt, name)
            if not (t.is_contiguous() and t.shape == in_ids.shape):
                raise _lib.UmvError(f"{who}: {name} must be a contiguous [max_len, B] tensor")
    if logits is not None:
        _req(logits, BF16, "logits")
        _logits_shape(who, logits, B)
    return B


def decode_step_end_argmax(tok_slot, tok_pos, kv_len, argmax_partial, ids, in_ids, pred_ids, step_idx):
    """ids = argmax over the per-tile keys the lm_head GEMM left in argmax_partial, then decode_step_end's bookkeeping.
    step_idx: one counter per sample ([B] int64, all equal)."""
    lib = _lib.load()
    B = _check_fused_step_end("decode_step_end_argmax", argmax_partial, ids, in_ids, pred_ids, step_idx)
    check(lib.umv_decode_step_end_argmax(_p(tok_slot), _p(tok_pos), _p(kv_len), _p(argmax_partial), argmax_partial.shape[1], _p(ids),
                                         _p(in_ids), _p(pred_ids), _p(step_idx), B, in_ids.shape[0], _stream()),
          "umv_decode_step_end_argmax")


def decode_step_end_logprob(tok_slot, tok_pos, kv_len, argmax_partial, lse_partial, ids, in_ids, pred_ids, step_idx, logits, logprobs,
                            temperature=0.0, forced_ids=None):
    """decode_step_end_argmax that also writes logprobs[s] (fp32 [max_len, B]): the log-probability of the token the next step is fed,
    from the per-tile softmax statistics the lm_head GEMM left in lse_partial ([B, n_tiles, 2]) and the logits it stored.  temperature:
    the one the GEMM sampled at, 0 = greedy.  forced_ids (int64 [max_len, B] or None): an entry >= 0 replaces the pick as ids /
    in_ids[s + 1] - and the log-probability is that token's - while pred_ids[s] keeps the model's own pick; negative = free-running."""
    lib = _lib.load()
    B = _check_fused_step_end("decode_step_end_logprob", argmax_partial, ids, in_ids, pred_ids, step_idx, lse_partial, logits,
                              logprobs=(logprobs, torch.float32), forced_ids=(forced_ids, torch.int64))
    check(lib.umv_decode_step_end_logprob(_p(tok_slot), _p(tok_pos), _p(kv_len), _p(argmax_partial), _p(lse_partial), argmax_partial.shape[1],
                                          _p(ids), _p(in_ids), _p(pred_ids), _p(step_idx), _p(logits), logits.stride(0), logits.shape[1],
                                          float(temperature), _p(forced_ids), _p(logprobs), B, in_ids.shape[0], _stream()),
          "umv_decode_step_end_logprob")


def decode_step_end_truncated(tok_slot, tok_pos, kv_len, argmax_partial, ids, in_ids, pred_ids, step_idx, logits, temperature, seed,
                              top_k=0, top_p=1.0, min_p=0.0, lse_partial=None, logprobs=None, forced_ids=None, cut_y=None, n_kept=None):
    """The step end of a truncated sampling step (include/unimedvl_hip.h): the pick is the lm_head sampling epilogue's (argmax_partial,
    sampled at the same temperature, seed and step_idx) where that column survives top-k / top-p / min-p, the Gumbel maximum over the kept
    columns under the same noise otherwise; then decode_step_end_logprob's bookkeeping.  lse_partial with logprobs, and forced_ids, as
    there; cut_y (fp32) / n_kept (int32), both [max_len, B], receive row s."""
    lib = _lib.load()
    if (lse_partial is None) != (logprobs is None):
        raise _lib.UmvError("decode_step_end_truncated: lse_partial and logprobs go together")
    B = _check_fused_step_end("decode_step_end_truncated", argmax_partial, ids, in_ids, pred_ids, step_idx, lse_partial, logits,
                              logprobs=(logprobs, torch.float32), forced_ids=(forced_ids, torch.int64), cut_y=(cut_y, torch.float32),
                              n_kept=(n_kept, torch.int32))
    check(lib.umv_decode_step_end_truncated(_p(tok_slot), _p(tok_pos), _p(kv_len), _p(argmax_partial), _p(lse_partial), argmax_partial.shape[1],
                                            _p(ids), _p(in_ids), _p(pred_ids), _p(step_idx), _p(logits), logits.stride(0), logits.shape[1],
                                            float(temperature), _p(forced_ids), _p(logprobs), B, in_ids.shape[0],
                                            _seed64(seed), int(top_k), float(top_p), float(min_p), _p(cut_y), _p(n_kept),
                                            _stream()),
          "umv_decode_step_end_truncated")


def decode_step_end_rows(tok_slot, tok_pos, kv_len, argmax_partial, ids, in_ids, pred_ids, step_idx, logits, sample_rows, lse_partial=None,
                         logprobs=None, forced_ids=None, cut_y=None, n_kept=None):
    """The step end of a step with a per-row sampling table (include/unimedvl_hip.h; sample_rows = sampling.to_tensor's int64 [B, 6],
    the table the lm_head call got): per row decode_step_end_truncated with the row's own temperature, filters and (seed, draw, stream)
    where the row samples with a filter on, the key maximum of decode_step_end_logprob otherwise (cut_y = -inf, n_kept = V).  Adds 1 to
    every row's draw counter - the only word of the table it writes.  lse_partial with logprobs, forced_ids, cut_y, n_kept as there."""
    lib = _lib.load()
    if (lse_partial is None) != (logprobs is None):
        raise _lib.UmvError("decode_step_end_rows: lse_partial and logprobs go together")
    B = _check_fused_step_end("decode_step_end_rows", argmax_partial, ids, in_ids, pred_ids, step_idx, lse_partial, logits,
                              logprobs=(logprobs, torch.float32), forced_ids=(forced_ids, torch.int64), cut_y=(cut_y, torch.float32),
                              n_kept=(n_kept, torch.int32))
    rows = None if sample_rows is None else _row_table(sample_rows, B, "decode_step_end_rows")
    check(lib.umv_decode_step_end_rows(_p(tok_slot), _p(tok_pos), _p(kv_len), _p(argmax_partial), _p(lse_partial), argmax_partial.shape[1],
                                       _p(ids), _p(in_ids), _p(pred_ids), _p(step_idx), _p(logits), logits.stride(0), logits.shape[1],
                                       _p(forced_ids), _p(logprobs), B, in_ids.shape[0], rows, _p(cut_y), _p(n_kept), _stream()),
          "umv_decode_step_end_rows")


def _spec_step_args(who, tok_slot, tok_pos, kv_len, argmax_partial, ids, out_ids, n_out, limit, n_draft, hist, hist_len, stats, draft_len,
                    vocab, ngram, predicted, pred_len, draft_only):
    """umv_spec_step_args from the tensors of a speculative step, checked (argmax_partial may be None where the entry does not read it)"""
    k, B = int(draft_len), kv_len.numel()
    T = B * (k + 1)
    n_tiles = (int(vocab) + 15) // 16
    i32 = [(tok_slot, "tok_slot", T), (tok_pos, "tok_pos", T), (kv_len, "kv_len", B), (n_out, "n_out", B), (limit, "limit", B),
           (n_draft, "n_draft", B), (hist_len, "hist_len", B), (stats, "stats", 3 * B), (hist, "hist", None)]
    if pred_len is not None:
        i32.append((pred_len, "pred_len", B))
    i64 = [(ids, "ids", T), (out_ids, "out_ids", None)]
    if argmax_partial is not None:
        i64.append((argmax_partial, "argmax_partial", T * n_tiles))
    if predicted is not None:
        i64.append((predicted, "predicted", None))
    for group, dt in ((i32, torch.int32), (i64, torch.int64)):
        for t, name, n in group:
            _req(t, dt, name)
            if not t.is_contiguous() or (n is not None and t.numel() != n) or (n is None and (t.dim() != 2 or t.shape[0] != B)):
                raise _lib.UmvError(f"{who}: {name} must be contiguous with {'[B, n]' if n is None else n} entries "
                                    f"(B = {B}, draft_len = {k}), got {tuple(t.shape)}")
    if (predicted is None) != (pred_len is None):
        raise _lib.UmvError(f"{who}: predicted and pred_len go together")
    return _lib.SpecStepArgs(
        tok_slot=tok_slot.data_ptr(), tok_pos=tok_pos.data_ptr(), kv_len=kv_len.data_ptr(),
        argmax_partial=None if argmax_partial is None else argmax_partial.data_ptr(),
        n_tiles=n_tiles, V=int(vocab), ids=ids.data_ptr(), out_ids=out_ids.data_ptr(), out_ld=out_ids.shape[1], n_out=n_out.data_ptr(),
        limit=limit.data_ptr(), n_draft=n_draft.data_ptr(), hist=hist.data_ptr(), hist_ld=hist.shape[1], hist_len=hist_len.data_ptr(),
        predicted=None if predicted is None else predicted.data_ptr(), pred_ld=0 if predicted is None else predicted.shape[1],
        pred_len=None if pred_len is None else pred_len.data_ptr(), stats=stats.data_ptr(), B=B, k=k, ngram_min=int(ngram[0]),
        ngram_max=int(ngram[1]), draft_only=int(bool(draft_only)))


def decode_step_end_speculative(tok_slot, tok_pos, kv_len, argmax_partial, ids, out_ids, n_out, limit, n_draft, hist, hist_len, stats,
                                draft_len, vocab, ngram=(2, 4), predicted=None, pred_len=None, draft_only=False):
    """The step end of a speculative greedy step (include/unimedvl_hip.h): per sample verify the draft_len drafts of this step's rows
    against the picks behind argmax_partial ([T, n_tiles], T = B * (draft_len + 1) rows), emit the accepted tokens plus one into
    out_ids [B, max] / n_out up to limit, advance slot / position / kv_len by as many, append them to hist / hist_len, draft the next
    rows (predicted [B, n] int64 + pred_len where a row has one, prompt lookup with ngram = (min, max) otherwise) and write them to
    ids / tok_slot / tok_pos [T] and n_draft; stats [B, 3] += (steps, drafted, accepted).  draft_only: only draft and write the rows."""
    lib = _lib.load()
    a = _spec_step_args("decode_step_end_speculative", tok_slot, tok_pos, kv_len, argmax_partial, ids, out_ids, n_out, limit, n_draft, hist,
                        hist_len, stats, draft_len, vocab, ngram, predicted, pred_len, draft_only)
    check(lib.umv_decode_step_end_speculative(C.byref(a), _stream()), "umv_decode_step_end_speculative")


def decode_pick_rows(argmax_partial, logits, sample_rows, picks, lse_partial=None, logprob=None, cut_y=None, n_kept=None):
    """Every row's pick with its own sampler and nothing else (include/unimedvl_hip.h, speculative decode with sampling): picks [T] int64
    from the keys the per-row lm_head call left in argmax_partial [T, n_tiles], the logits [T, V] it stored and the table sample_rows
    (sampling.to_tensor, [T, 6]) - decode_step_end_rows' pick, without its bookkeeping and without touching the table.  logprob (fp32
    [T], with lse_partial [T, n_tiles, 2]): the pick's own log-probability; cut_y (fp32 [T]) / n_kept (int32 [T]): the row's cutoff."""
    lib = _lib.load()
    _req(logits, BF16, "logits")
    _req(picks, torch.int64, "picks")
    T = picks.numel()
    if (lse_partial is None) != (logprob is None):
        raise _lib.UmvError("decode_pick_rows: lse_partial and logprob go together")
    if not picks.is_contiguous():
        raise _lib.UmvError("decode_pick_rows: picks must be a contiguous int64 [T] tensor")
    _, V = _logits_shape("decode_pick_rows", logits, T)
    _, _, rows, n_tiles = _tile_keys("decode_pick_rows", T, argmax_partial, lse_partial, sample_rows)
    _row_outputs("decode_pick_rows", T, logprob=(logprob, torch.float32), cut_y=(cut_y, torch.float32), n_kept=(n_kept, torch.int32))
    check(lib.umv_decode_pick_rows(_p(argmax_partial), _p(lse_partial), n_tiles, _p(logits), logits.stride(0), V, rows, T, _p(picks),
                                   _p(logprob), _p(cut_y), _p(n_kept), _stream()), "umv_decode_pick_rows")


def decode_step_end_speculative_rows(tok_slot, tok_pos, kv_len, picks, sample_rows, ids, out_ids, n_out, limit, n_draft, hist, hist_len, stats,
                                     draft_len, vocab, ngram=(2, 4), predicted=None, pred_len=None, draft_only=False, row_logprob=None,
                                     out_logprobs=None):
    """The commit launch of a sampled speculative step: decode_step_end_speculative whose picks are read from picks [T] (decode_pick_rows)
    instead of key maxima, which also sets the draw counters of the sample's table rows to d0 + m + j (m tokens emitted, row j) and, with
    row_logprob [T] / out_logprobs [B, max] (both or neither), copies the emitted tokens' log-probabilities next to out_ids.
    draft_only: only draft and write the rows; the table and the log-probabilities are not touched."""
    lib = _lib.load()
    who = "decode_step_end_speculative_rows"
    step = _spec_step_args(who, tok_slot, tok_pos, kv_len, None, ids, out_ids, n_out, limit, n_draft, hist, hist_len, stats, draft_len, vocab,
                           ngram, predicted, pred_len, draft_only)
    T = ids.numel()
    _req(picks, torch.int64, "picks")
    if not (picks.is_contiguous() and picks.numel() == T):
        raise _lib.UmvError(f"{who}: picks must be a contiguous tensor of {T} entries")
    if (row_logprob is None) != (out_logprobs is None):
        raise _lib.UmvError(f"{who}: row_logprob and out_logprobs go together")
    if row_logprob is not None:
        _req(row_logprob, torch.float32, "row_logprob")
        _req(out_logprobs, torch.float32, "out_logprobs")
        if not (row_logprob.is_contiguous() and row_logprob.numel() == T and out_logprobs.is_contiguous()
                and out_logprobs.shape == out_ids.shape):
            raise _lib.UmvError(f"{who}: row_logprob [{T}] and out_logprobs {tuple(out_ids.shape)} (as out_ids), contiguous")
    a = _lib.SpecRowsStepArgs(step=step, picks=picks.data_ptr(), rows=_row_table(sample_rows, T, who), row_logprob=None if row_logprob is None else row_logprob.data_ptr(),
                              out_logprobs=None if out_logprobs is None else out_logprobs.data_ptr())
    check(lib.umv_decode_step_end_speculative_rows(C.byref(a), _stream()), "umv_decode_step_end_speculative_rows")


def token_logprob(logits, ids, temperature=0.0, out=None):
    """out[m] = log_softmax(y[m])[ids[m]] in fp32 for bf16 logits [M, V] (any row stride): y = the logits (temperature 0: greedy) or
    bf16(logits / temperature), the value sampling orders.  For callers who hold logits - return_logits=True, a prefill's last rows."""
    lib = _lib.load()
    _req(logits, BF16, "logits")
    M, V = _logits_shape("token_logprob", logits)
    out = torch.empty((M,), dtype=torch.float32, device=logits.device) if out is None else out
    _row_outputs("token_logprob", M, ids=(ids, torch.int64), out=(out, torch.float32))
    check(lib.umv_token_logprob_bf16(_p(logits), logits.stride(0), _p(ids), _p(out), M, V, float(temperature), _stream()),
          "umv_token_logprob_bf16")
    return out


def lm_head_stats(x, lin, ids, lse_partial, target_y, *, M=None, use_bias=True):
    """The lm_head GEMM of the prefill-time scorer (include/unimedvl_hip.h, umv_lm_head_stats_bf16): for rows [0, M) of x [>= M, K] bf16
    the softmax statistics of every 16-column tile go to lse_partial (fp32 [>= M, ceil(N/16), 2]) and row m's logit at ids[m] (int64
    [>= M]) to target_y (fp32 [>= M]); no logits are stored.  Any M >= 1; the linear must hold its plain 16-row bf16 image - an e4m3 or
    MXFP4 lm_head takes gemm + token_logprob instead (Qwen2MoT.token_logprobs).  Finished by token_logprob_from_stats."""
    lib = _lib.load()
    _req(x, BF16, "x")
    assert x.stride(-1) == 1
    M = x.shape[0] if M is None else M
    if lin.wp is None or lin.th != 16 or lin.swiglu or lin.w8 is not None or lin.w4 is not None:
        raise _lib.UmvError("lm_head_stats needs a plain bf16 linear (16-row image, no SwiGLU, no e4m3 / MXFP4 image)")
    nt = (lin.N + 15) // 16
    _req(lse_partial, torch.float32, "lse_partial")
    if not (lse_partial.is_contiguous() and lse_partial.dim() == 3 and lse_partial.shape[0] >= M and lse_partial.shape[1:] == (nt, 2)):
        raise _lib.UmvError(f"lm_head_stats: lse_partial must be a contiguous fp32 [>= {M}, {nt}, 2] tensor")
    for name, t, dt in (("ids", ids, torch.int64), ("target_y", target_y, torch.float32)):
        _req(t, dt, name)
        if not (t.is_contiguous() and t.dim() == 1 and t.shape[0] >= M):
            raise _lib.UmvError(f"lm_head_stats: {name} must be a contiguous {dt} tensor of >= {M} entries")
    if x.shape[0] < M or x.shape[1] != lin.K:
        raise _lib.UmvError(f"lm_head_stats: x must be [>= {M}, {lin.K}]")
    a = GemmArgs(x=x.data_ptr(), ldx=x.stride(0), wp=lin.wp.data_ptr(), M=M, N=lin.N, K=lin.K, tile_rows=lin.th)
    if lin.bias is not None and use_bias:
        a.bias, a.epilogue = lin.bias.data_ptr(), EPI_BIAS
    check(lib.umv_lm_head_stats_bf16(C.byref(a), _p(ids), _p(lse_partial), _p(target_y), _stream()), "umv_lm_head_stats_bf16")


def token_logprob_from_stats(lse_partial, target_y, ids, V, out=None, *, M=None):
    """out[m] = target_y[m] - logsumexp of row m from its tile statistics (lm_head_stats' outputs), merged in decode_step_end_logprob's
    order: fp32 [M]; NaN where ids[m] lies outside [0, V)."""
    lib = _lib.load()
    _req(lse_partial, torch.float32, "lse_partial")
    if not (lse_partial.is_contiguous() and lse_partial.dim() == 3 and lse_partial.shape[2] == 2):
        raise _lib.UmvError("token_logprob_from_stats: lse_partial must be a contiguous fp32 [M, n_tiles, 2] tensor")
    M = lse_partial.shape[0] if M is None else M
    out = torch.empty((M,), dtype=torch.float32, device=lse_partial.device) if out is None else out
    for name, t, dt in (("ids", ids, torch.int64), ("target_y", target_y, torch.float32), ("out", out, torch.float32)):
        _req(t, dt, name)
        if not (t.is_contiguous() and t.dim() == 1 and t.shape[0] >= M):
            raise _lib.UmvError(f"token_logprob_from_stats: {name} must be a contiguous {dt} tensor of >= {M} entries")
    if lse_partial.shape[0] < M:
        raise _lib.UmvError(f"token_logprob_from_stats: lse_partial holds {lse_partial.shape[0]} rows, M = {M}")
    check(lib.umv_token_logprob_from_stats(_p(lse_partial), lse_partial.shape[1], _p(target_y), _p(ids), int(V), _p(out), M, _stream()),
          "umv_token_logprob_from_stats")
    return out


def check_top_logprobs(n, vocab=None):
    """The number of alternatives per token as an int: 0 = off, at most _lib.TOP_LOGPROBS_MAX and the vocabulary; ValueError otherwise."""
    if isinstance(n, bool) or int(n) != n or n < 0 or n > _lib.TOP_LOGPROBS_MAX:
        raise ValueError(f"top_logprobs must be an integer in [0, {_lib.TOP_LOGPROBS_MAX}] (0 = off), got {n!r}")
    if vocab is not None and n > vocab:
        raise ValueError(f"top_logprobs ({n}) exceeds the vocabulary ({vocab})")
    return int(n)


def _top_n(who, n, V):
    if isinstance(n, bool) or int(n) != n or not 1 <= n <= min(_lib.TOP_LOGPROBS_MAX, V):
        raise _lib.UmvError(f"{who}: n must be an integer in [1, {_lib.TOP_LOGPROBS_MAX}] and at most V = {V}, got {n!r}")
    return int(n)


def decode_top_logprobs(logits, lse_partial, ids, step_idx, top_ids, top_logprobs, rank, temperature=0.0, sample_rows=None,
                        truncated=False, forced_ids=None):
    """After a fused step end (include/unimedvl_hip.h, top-n alternative tokens): row s = step_idx - 1 of top_ids (int32 [max_len, B, n]),
    top_logprobs (fp32, same shape) and rank (int32 [max_len, B]) - the n best columns of every sample by (y descending, column
    ascending) with their log-probabilities, and the 1-based rank of the token the step end left in ids.  logits / lse_partial /
    temperature / sample_rows / forced_ids: what the step end got; truncated: the step end was decode_step_end_truncated (the order its
    statistics were merged in; with sample_rows the row's own is taken)."""
    lib = _lib.load()
    _req(logits, BF16, "logits")
    _req(ids, torch.int64, "ids")
    _req(step_idx, torch.int64, "step_idx")
    _req(top_ids, torch.int32, "top_ids")
    _req(top_logprobs, torch.float32, "top_logprobs")
    _req(rank, torch.int32, "rank")
    B = ids.numel()
    if top_ids.dim() != 3:
        raise _lib.UmvError("decode_top_logprobs: top_ids must be [max_len, B, n]")
    max_len, _, n = top_ids.shape
    _, V = _logits_shape("decode_top_logprobs", logits, B)
    n = _top_n("decode_top_logprobs", n, V)
    if not (top_ids.is_contiguous() and top_logprobs.is_contiguous() and rank.is_contiguous() and tuple(top_ids.shape) == (max_len, B, n)
            and top_logprobs.shape == top_ids.shape and tuple(rank.shape) == (max_len, B) and ids.is_contiguous() and step_idx.numel() >= B):
        raise _lib.UmvError("decode_top_logprobs: top_ids / top_logprobs [max_len, B, n], rank [max_len, B], ids [B], step_idx [B], all contiguous")
    _, _, rows, n_tiles = _tile_keys("decode_top_logprobs", B, None, _req(lse_partial, torch.float32, "lse_partial"), sample_rows)
    if forced_ids is not None:
        _req(forced_ids, torch.int64, "forced_ids")
        if not (forced_ids.is_contiguous() and tuple(forced_ids.shape) == (max_len, B)):
            raise _lib.UmvError("decode_top_logprobs: forced_ids must be a contiguous [max_len, B] tensor")
    order = _lib.TOP_AFTER_TRUNCATED if truncated else _lib.TOP_AFTER_LOGPROB
    check(lib.umv_decode_top_logprobs(_p(logits), logits.stride(0), V, _p(lse_partial), n_tiles, float(temperature), rows, order,
                                      _p(ids), _p(step_idx), _p(forced_ids), B, max_len, n, _p(top_ids), _p(top_logprobs), _p(rank),
                                      _stream()),
          "umv_decode_top_logprobs")


def top_logprobs(logits, ids, n, temperature=0.0):
    """The n best columns of every row of bf16 logits [M, V] (any row stride) by (y descending, column ascending), y as token_logprob's:
    (top_ids int32 [M, n], top_logprobs fp32 [M, n], rank int32 [M]) - rank the 1-based place of ids[m] in that order, 0 for an id outside
    the vocabulary.  Where ids[m] is among the n, its entry is token_logprob's value bit for bit."""
    M, V = _logits_shape("top_logprobs", logits)
    if not (ids.is_contiguous() and ids.numel() == M):
        raise _lib.UmvError("top_logprobs: ids must be a contiguous int64 [M] tensor")
    n = _top_n("top_logprobs", n, V)                    # (refused on the host, before anything touches the library)
    lib = _lib.load()
    _req(logits, BF16, "logits")
    _req(ids, torch.int64, "ids")
    top_ids = torch.empty((M, n), dtype=torch.int32, device=logits.device)
    top_lp = torch.empty((M, n), dtype=torch.float32, device=logits.device)
    rank = torch.empty((M,), dtype=torch.int32, device=logits.device)
    check(lib.umv_top_logprobs_bf16(_p(logits), logits.stride(0), _p(ids), M, V, float(temperature), n, _p(top_ids), _p(top_lp), _p(rank),
                                    _stream()),
          "umv_top_logprobs_bf16")
    return top_ids, top_lp, rank


# ----------------------------------------------------------------------------- beam search decode (include/unimedvl_hip.h)
def check_beams(num_beams, vocab=None, rows=None):
    """The beams per request as an int: 1 = off, at most _lib.BEAM_K_MAX, the vocabulary larger than 2K and - rows the request count -
    at most 64 rows in all; ValueError otherwise."""
    if isinstance(num_beams, bool) or int(num_beams) != num_beams or not 1 <= num_beams <= _lib.BEAM_K_MAX:
        raise ValueError(f"num_beams must be an integer in [1, {_lib.BEAM_K_MAX}] (1 = off), got {num_beams!r}")
    K = int(num_beams)
    if K > 1 and vocab is not None and vocab <= 2 * K:
        raise ValueError(f"num_beams = {K} needs a vocabulary of more than {2 * K} tokens (got {vocab})")
    if K > 1 and rows is not None and rows * K > 64:
        raise ValueError(f"beam search decode serves at most 64 rows per step: {rows} requests x {K} beams")
    return K


def beam_candidates(logits, lse_partial, cand_ids, cand_lp, rank):
    """cand_ids (int32) / cand_lp (fp32) [R, 2K]: every row's 2K best columns by (bf16 logit descending, column ascending) with their
    log-probabilities - the greedy top-n list of decode_top_logprobs, bit for bit.  rank: int32 [R] scratch."""
    lib = _lib.load()
    _req(logits, BF16, "logits")
    _req(cand_ids, torch.int32, "cand_ids")
    _req(cand_lp, torch.float32, "cand_lp")
    _req(rank, torch.int32, "rank")
    if cand_ids.dim() != 2 or cand_lp.shape != cand_ids.shape or not (cand_ids.is_contiguous() and cand_lp.is_contiguous()):
        raise _lib.UmvError("beam_candidates: cand_ids / cand_lp must be contiguous [R, 2K] tensors of one shape")
    R, n = cand_ids.shape
    _, V = _logits_shape("beam_candidates", logits, R)
    if n % 2 or not 2 <= n <= 2 * _lib.BEAM_K_MAX or V <= n or rank.numel() < R or not rank.is_contiguous():
        raise _lib.UmvError(f"beam_candidates: 2K = {n} must be even, at most {2 * _lib.BEAM_K_MAX} and below V = {V}; rank holds R entries")
    _, lse, _, n_tiles = _tile_keys("beam_candidates", R, None, _req(lse_partial, torch.float32, "lse_partial"))
    check(lib.umv_beam_candidates(_p(logits), logits.stride(0), V, lse, n_tiles, R, n, _p(cand_ids), _p(cand_lp), _p(rank), _stream()),
          "umv_beam_candidates")


class BeamState:
    """The device words of a beam search (umv_beam_step_args) for B requests of K beams: scores, back-pointers, finished list, done
    words and copy list - allocated here - next to the decode session's counters and the forked cache's table."""

    def __init__(self, B, K, max_length, device, length_penalty=1.0):
        R = B * K
        self.B, self.K, self.max_length = B, K, max_length
        self.cand_ids = torch.zeros((R, 2 * K), dtype=torch.int32, device=device)
        self.cand_lp = torch.zeros((R, 2 * K), dtype=torch.float32, device=device)
        self.rank = torch.zeros((R,), dtype=torch.int32, device=device)
        scores = torch.full((B, K), float("-inf"), dtype=torch.float32)
        scores[:, 0] = 0.0
        self.scores = scores.reshape(R).to(device)
        self.beam_tok = torch.zeros((max_length, R), dtype=torch.int32, device=device)
        self.beam_parent = torch.zeros((max_length, R), dtype=torch.int32, device=device)
        self.beam_lp = torch.zeros((max_length, R), dtype=torch.float32, device=device)
        self.fin_f = torch.zeros((B, K, 4), dtype=torch.float32, device=device)
        self.fin_i = torch.zeros((B, K, 4), dtype=torch.int32, device=device)
        self.hdr = torch.zeros((B, 4), dtype=torch.int32, device=device)
        self.copies = torch.zeros((R, 4), dtype=torch.int32, device=device)
        # norm[t] = powf(t + 1, length_penalty) in fp32, once, on the host: the device divides by it
        import numpy as np
        norm = np.power(np.arange(1, max_length + 1, dtype=np.float32), np.float32(length_penalty)).astype(np.float32)
        self.len_norm = torch.from_numpy(norm).to(device)

    def written(self):
        """every tensor a step end writes that a later one (or the copy launch) reads"""
        return (self.scores, self.fin_f, self.fin_i, self.hdr, self.copies)


def beam_step_end(tok_slot, tok_pos, kv_len, ids, step_idx, st, table, own, j0, end_token_id, early_stopping):
    """The step end of a beam search step (include/unimedvl_hip.h, beam search decode) over st (a BeamState, its candidate lists
    filled by beam_candidates): orders and walks the candidates of every request, keeps its finished list and done word, writes the
    next ids, back-pointers and scores, advances the counters, rewrites the request's rows of `table` (int32 [R, stride]) by the KV plan
    and leaves st.copies.  own (int32 [R, n_own, 2]) / j0 (int32 [B]): kvcache.PagedCache.fork_beams."""
    lib = _lib.load()
    R = st.B * st.K
    for t, dt, name, numel in ((tok_slot, torch.int32, "tok_slot", R), (tok_pos, torch.int32, "tok_pos", R), (kv_len, torch.int32, "kv_len", R),
                               (ids, torch.int64, "ids", R), (step_idx, torch.int64, "step_idx", R), (j0, torch.int32, "j0", st.B)):
        _req(t, dt, name)
        if not (t.is_contiguous() and t.numel() >= numel):
            raise _lib.UmvError(f"beam_step_end: {name} must be a contiguous tensor of {numel} entries")
    _req(table, torch.int32, "table")
    _req(own, torch.int32, "own")
    if not (table.dim() == 2 and table.shape[0] == R and table.stride(1) == 1 and own.is_contiguous() and own.dim() == 3
            and own.shape[0] == R and own.shape[2] == 2):
        raise _lib.UmvError(f"beam_step_end: table must be int32 [{R}, stride] and own a contiguous int32 [{R}, n_own, 2]")
    if st.K * own.shape[1] > _lib.BEAM_TABLE_ENTRIES:
        raise _lib.UmvError(f"beam_step_end: K * n_own = {st.K * own.shape[1]} exceeds {_lib.BEAM_TABLE_ENTRIES}: shorten the decode horizon")
    a = _lib.BeamStepArgs()
    a.tok_slot, a.tok_pos, a.kv_len, a.ids, a.step_idx = (t.data_ptr() for t in (tok_slot, tok_pos, kv_len, ids, step_idx))
    a.cand_ids, a.cand_lp, a.scores = st.cand_ids.data_ptr(), st.cand_lp.data_ptr(), st.scores.data_ptr()
    a.beam_tok, a.beam_parent, a.beam_lp = st.beam_tok.data_ptr(), st.beam_parent.data_ptr(), st.beam_lp.data_ptr()
    a.fin_f, a.fin_i, a.hdr, a.len_norm = st.fin_f.data_ptr(), st.fin_i.data_ptr(), st.hdr.data_ptr(), st.len_norm.data_ptr()
    a.table, a.own, a.j0, a.copies = table.data_ptr(), own.data_ptr(), j0.data_ptr(), st.copies.data_ptr()
    a.table_stride, a.n_own, a.B, a.K, a.max_len = table.stride(0), own.shape[1], st.B, st.K, st.max_length
    a.end_token_id, a.early_stopping = -1 if end_token_id is None else int(end_token_id), int(bool(early_stopping))
    check(lib.umv_beam_step_end(C.byref(a), _stream()), "umv_beam_step_end")


def beam_pool_pointers(slabs):
    """the device array umv_beam_kv_copy takes: per layer the K pool's and the V^T pool's base address (int64 [2 * layers])"""
    ptrs = [p for sl in slabs for p in (sl.k.data_ptr(), sl.vt.data_ptr())]
    return torch.tensor(ptrs, dtype=torch.int64).to(slabs[0].k.device)


def beam_kv_copy(copies, pools, slabs, chunks=4):
    """Carry out a step end's copy list (int32 [R, 4]) in every layer's pools: the first `tokens` slots of the source page into the
    destination page, K and V^T of every kv head.  pools: beam_pool_pointers(slabs)."""
    lib = _lib.load()
    _req(copies, torch.int32, "copies")
    _req(pools, torch.int64, "pools")
    sl = slabs[0]
    if not (copies.is_contiguous() and copies.dim() == 2 and copies.shape[1] == 4 and pools.numel() == 2 * len(slabs)):
        raise _lib.UmvError("beam_kv_copy: copies must be a contiguous int32 [R, 4] and pools hold two pointers per layer")
    check(lib.umv_beam_kv_copy(_p(copies), _p(pools), copies.shape[0], len(slabs), sl.nkv, sl.hd, sl.k.shape[0], int(chunks), _stream()),
          "umv_beam_kv_copy")


def timestep_embed(t, freqs):
    """[n] fp32 timesteps (device) x [half] fp32 frequencies -> [n, 2*half] bf16 sinusoid (cos | sin)"""
    lib = _lib.load()
    _req(t, torch.float32, "t")
    _req(freqs, torch.float32, "freqs")
    n, half = t.numel(), freqs.numel()
    out = torch.empty((n, 2 * half), dtype=BF16, device=t.device)
    check(lib.umv_timestep_embed(_p(t), _p(freqs), _p(out), n, half, _stream()), "umv_timestep_embed")
    return out


def cfg_renorm_euler(x_t, v_t, v_text, v_img, rows, seg_off, nseg, s_text, s_img, renorm_min, rtype, dt):
    lib = _lib.load()
    _req(x_t, torch.float32, "x_t")
    _req(v_t, BF16, "v_t")
    check(lib.umv_cfg_renorm_euler(_p(x_t), _p(v_t), _p(v_text), _p(v_img), v_t.stride(0), _p(rows), _p(seg_off), nseg,
                                   float(s_text), float(s_img), float(renorm_min), int(rtype), float(dt), x_t.shape[1],
                                   _stream()), "umv_cfg_renorm_euler")
