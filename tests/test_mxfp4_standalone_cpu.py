"""The fp4 mode without bf16 images (llm_fp4_keep_bf16=False), host side: config validation, the packed file's tag, and the C ABI of
the tiled MXFP4 GEMM (header declaration, ctypes binding, sanitizer driver)."""
import os
import re

import pytest

from unimedvl_amd.config import UniMedVLConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_field_defaults_to_the_carried_mode_and_round_trips():
    c = UniMedVLConfig()
    assert c.llm_fp4_keep_bf16 is True
    d = UniMedVLConfig(llm_weight_dtype="fp4", llm_fp4_keep_bf16=False).to_dict()
    assert d["llm_fp4_keep_bf16"] is False
    c2 = UniMedVLConfig.from_dict(d)
    assert c2.llm_fp4_keep_bf16 is False and c2.llm_weight_dtype == "fp4" and c2.to_dict() == d
    assert UniMedVLConfig.from_dict({"llm_weight_dtype": "fp4"}).llm_fp4_keep_bf16 is True


def test_standalone_needs_fp4_weights():
    from unimedvl_amd.weights import check_llm_dtypes
    check_llm_dtypes(UniMedVLConfig(llm_weight_dtype="fp4", llm_fp4_keep_bf16=False))
    check_llm_dtypes(UniMedVLConfig(llm_weight_dtype="fp4", llm_fp4_keep_bf16=True))
    for wd, ad in (("bf16", "bf16"), ("fp8", "bf16"), ("fp8", "fp8")):
        check_llm_dtypes(UniMedVLConfig(llm_weight_dtype=wd, llm_act_dtype=ad))
        with pytest.raises(ValueError, match="llm_fp4_keep_bf16"):
            check_llm_dtypes(UniMedVLConfig(llm_weight_dtype=wd, llm_act_dtype=ad, llm_fp4_keep_bf16=False))


def test_packed_file_tag_differs(tmp_path):
    from unimedvl_amd import packstore
    paths = {}
    for keep in (True, False):
        cfg = UniMedVLConfig(llm_weight_dtype="fp4", llm_fp4_keep_bf16=keep)
        store = packstore.attach(lambda n: None, str(tmp_path), "cpu", cfg, [], enabled=False, extra_tag="_und")
        paths[keep] = (os.path.basename(store.path), store.dtype_tag)
    assert paths[True] == ("ema_packed_w-fp4_a-bf16_und.safetensors", "w-fp4_a-bf16_und")
    assert paths[False][0] != paths[True][0] and paths[False][1] != paths[True][1]
    assert paths[False][0].startswith("ema_packed_w-fp4_a-bf16") and paths[False][0].endswith("_und.safetensors")


def test_header_declares_and_ctypes_binds_the_tiled_entry():
    from unimedvl_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "unimedvl_hip.h")).read()
    assert re.search(r"\bint\s+umv_gemm_mxfp4t\s*\(\s*const\s+umv_gemm_args\s*\*\s*\w*\s*,\s*umv_stream_t\s+\w*\s*\)\s*;", hdr)
    assert "umv_gemm_mxfp4t" in _lib._SIGS and _lib._SIGS["umv_gemm_mxfp4t"] == _lib._SIGS["umv_gemm_mxfp4w"]
    from unimedvl_amd import build
    assert "gemm_mxfp4t.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "gemm_mxfp4t.hip"))
    drv = open(os.path.join(ROOT, "tools", "abi_sanitize_driver.cpp")).read()
    assert "umv_gemm_mxfp4t(" in drv


def test_packer_sources_are_untouched_by_name():
    """the packed files' layout stamp covers pack.hip and quant.h: the tiled kernel reads the image those make, it has no packer of its own"""
    from unimedvl_amd import packstore
    assert "csrc/pack.hip" in packstore.PACK_SOURCES and "csrc/quant.h" in packstore.PACK_SOURCES
    src = open(os.path.join(ROOT, "unimedvl_amd", "csrc", "gemm_mxfp4t.hip")).read()
    assert "cvt_fp4x8" in src and "e8m0_scale" in src and "gemm_epilogue.h" in src
