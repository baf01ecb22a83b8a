"""Per-request sampling parameters on the host: SamplingParams validation, the packing of a list of params into the per-row table, and
the table's layout - the numpy dtype and the ctypes mirror against the C struct of include/unimedvl_hip.h as the host compiler lays it
out (the probe is built the way tests/test_abi_layout_cpu.py builds its own)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "unimedvl_hip.h")
INCLUDE = os.path.join(ROOT, "include")
FIELDS = ["seed", "draw", "stream", "temperature", "top_k", "top_p", "min_p", "repetition_penalty", "presence_penalty", "frequency_penalty"]


def _c_layout(tmp_path, structs):
    """{struct: {field or 'size': offset}} from a C program compiled from the header"""
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {"]
    for cs, fields in structs.items():
        lines.append(f'  printf("{cs} size %zu\\n", sizeof({cs}));')
        for f in fields:
            lines.append(f'  printf("{cs} {f} %zu\\n", offsetof({cs}, {f}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "rows_abi.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "rows_abi"
    subprocess.check_call(["gcc", "-std=c11", f"-I{INCLUDE}", "-o", str(exe), str(src)])
    c = {}
    for ln in subprocess.check_output([str(exe)], text=True).splitlines():
        s, f, v = ln.split()
        c.setdefault(s, {})[f] = int(v)
    return c


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_the_table_layout_is_the_c_struct(tmp_path):
    from unimedvl_amd import _lib, sampling
    c = _c_layout(tmp_path, {"umv_row_sampling": FIELDS, "umv_gemm_args": ["lse_partial"], "umv_logit_penalty_args": ["step", "rows"]})
    row = c["umv_row_sampling"]
    assert row["size"] == 48, "the issue fixes the row at 48 bytes"
    dt = sampling.ROW_DTYPE
    assert dt.itemsize == row["size"] and list(dt.names) == FIELDS
    assert ctypes.sizeof(_lib.RowSampling) == row["size"] and [n for n, _ in _lib.RowSampling._fields_] == FIELDS
    for f in FIELDS:
        assert dt.fields[f][1] == row[f], f"{f}: offset {row[f]} in C, {dt.fields[f][1]} in the numpy dtype"
        assert getattr(_lib.RowSampling, f).offset == row[f], f"{f}: offset {row[f]} in C, {getattr(_lib.RowSampling, f).offset} in ctypes"
        assert dt.fields[f][0].itemsize == ctypes.sizeof(dict(_lib.RowSampling._fields_)[f])
    assert dt.fields["seed"][0] == np.uint64 and dt.fields["draw"][0] == np.int64 and dt.fields["stream"][0] == np.uint32
    assert dt.fields["top_k"][0] == np.int32 and all(dt.fields[f][0] == np.float32 for f in FIELDS[3:] if f != "top_k")
    # the penalty struct gained its trailing pointer; the GEMM struct - a kernel argument of every GEMM - is as it was, the table goes
    # to the *_rows entries behind it
    for cs, cls, last in (("umv_gemm_args", _lib.GemmArgs, "lse_partial"), ("umv_logit_penalty_args", _lib.LogitPenaltyArgs, "rows")):
        assert cls._fields_[-1][0] == last and getattr(cls, last).offset == c[cs][last] and ctypes.sizeof(cls) == c[cs]["size"]
    for name, n in (("umv_gemm_bf16_rows", 3), ("umv_gemm_fp8w_rows", 3), ("umv_gemm_z13w_rows", 4)):
        assert len(_lib._SIGS[name][1]) == n


def test_packing():
    from unimedvl_amd import sampling
    from unimedvl_amd.sampling import SamplingParams
    ps = [SamplingParams(), SamplingParams(do_sample=True, temperature=0.7, top_k=5, top_p=0.9, min_p=0.05, seed=2 ** 63 + 11),
          SamplingParams(repetition_penalty=1.3, presence_penalty=0.5, frequency_penalty=-0.25),
          SamplingParams(do_sample=False, temperature=0.7)]
    t = sampling.pack(ps, seed=77, streams=[0, 5, 2 ** 32 - 1, 3], draws=[0, 9, 0, 2 ** 40])
    assert t.dtype == sampling.ROW_DTYPE and t.shape == (4,)
    # do_sample=False packs temperature 0 and neutral filters, whatever the params' temperature
    assert t["temperature"].tolist() == [0.0, np.float32(0.7), 0.0, 0.0]
    assert t["top_k"].tolist() == [0, 5, 0, 0] and t["top_p"].tolist() == [1.0, np.float32(0.9), 1.0, 1.0]
    assert t["min_p"].tolist() == [0.0, np.float32(0.05), 0.0, 0.0]
    # the seed: the params' own, or the one given to pack
    assert t["seed"].tolist() == [77, 2 ** 63 + 11, 77, 77]
    assert t["stream"].tolist() == [0, 5, 2 ** 32 - 1, 3] and t["draw"].tolist() == [0, 9, 0, 2 ** 40]
    assert t["repetition_penalty"].tolist() == [1.0, 1.0, np.float32(1.3), 1.0]
    assert t["presence_penalty"].tolist() == [0.0, 0.0, 0.5, 0.0] and t["frequency_penalty"].tolist() == [0.0, 0.0, -0.25, 0.0]
    # the bytes, through the ctypes mirror of the C struct
    from unimedvl_amd import _lib
    row = _lib.RowSampling.from_buffer_copy(t[1:2].tobytes())
    assert (row.seed, row.draw, row.stream, row.top_k) == (2 ** 63 + 11, 9, 5, 5) and row.temperature == np.float32(0.7)
    # the device form: int64 words, six per row, column 1 the draw counter
    words = sampling.to_tensor(t, "cpu")
    assert tuple(words.shape) == (4, 6) and words[:, 1].tolist() == [0, 9, 0, 2 ** 40]
    assert sampling.from_tensor(words).tobytes() == t.tobytes()
    assert sampling.pack([]).shape == (0,)
    with pytest.raises(ValueError):
        sampling.pack(ps, streams=[0])
    with pytest.raises(ValueError):
        sampling.pack_row(ps[0], draw=-1)
    with pytest.raises(ValueError):
        sampling.pack_row(ps[0], stream=2 ** 32)
    with pytest.raises(ValueError):
        sampling.pack_row(dict(temperature=1.0))


def test_validation():
    from unimedvl_amd.sampling import SamplingParams
    SamplingParams(do_sample=True, temperature=0.01, top_k=1, top_p=1.0, min_p=0.0)
    SamplingParams(do_sample=False, temperature=0.0)            # a greedy request may carry any finite temperature: it is not used
    bad = [dict(do_sample=True, temperature=0.0), dict(do_sample=True, temperature=-1.0), dict(do_sample=True, temperature=float("nan")),
           dict(temperature=float("inf")), dict(temperature="1"), dict(do_sample=1),
           dict(top_k=3), dict(top_p=0.9), dict(min_p=0.1),                                   # filters without a sampler
           dict(do_sample=True, top_k=-1), dict(do_sample=True, top_k=1.5), dict(do_sample=True, top_p=0.0),
           dict(do_sample=True, top_p=1.5), dict(do_sample=True, min_p=1.0), dict(do_sample=True, min_p=-0.1),
           dict(repetition_penalty=0.0), dict(repetition_penalty=float("inf")), dict(presence_penalty=float("nan")),
           dict(frequency_penalty=float("inf")), dict(seed=1.5), dict(seed=True)]
    for kw in bad:
        with pytest.raises(ValueError):
            SamplingParams(**kw)
    p = SamplingParams(do_sample=True, temperature=1, top_k=4)
    assert isinstance(p.temperature, float) and p.truncated and not p.penalised
    assert SamplingParams(presence_penalty=0.5).penalised and not SamplingParams(do_sample=True).truncated


def test_derived_seeds_are_a_function_of_the_request():
    from unimedvl_amd.sampling import derive_seed
    a = [derive_seed(1234, rid) for rid in range(64)]
    assert a == [derive_seed(1234, rid) for rid in range(64)] and len(set(a)) == 64 and all(0 <= s < 2 ** 64 for s in a)
    assert derive_seed(1235, 0) != a[0]


def test_the_session_and_the_batcher_refuse_mixed_keywords():
    """row_sampling excludes the scalar sampler keywords; the refusals come before anything touches a device"""
    from unimedvl_amd.decode import DecodeSession
    from unimedvl_amd.sampling import SamplingParams
    rows = [SamplingParams()]
    for kw in (dict(do_sample=True), dict(temperature=0.7), dict(top_k=3), dict(top_p=0.9), dict(min_p=0.1), dict(repetition_penalty=1.2),
               dict(presence_penalty=0.1), dict(frequency_penalty=0.1)):
        with pytest.raises(ValueError, match="row_sampling excludes"):
            DecodeSession(None, None, None, None, 4, row_sampling=rows, **kw)
    with pytest.raises(ValueError, match="go with row_sampling"):
        DecodeSession(None, None, None, None, 4, row_streams=[0])
    with pytest.raises(ValueError, match="go with row_sampling"):
        DecodeSession(None, None, None, None, 4, row_penalties=True)
