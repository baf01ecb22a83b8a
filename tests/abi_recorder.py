"""The C ABI behind three seams, for tests that pin which library calls the Python layer makes without a GPU or the shared library
(test_gemm_routing_cpu.py, test_decode_step_calls_cpu.py): _lib.load returns a recorder (every attribute a function that logs
(name, args) and returns 0), ops._stream returns None, ops._req checks the dtype only.  CPU tensors then flow through unchanged, and
render() turns the log into text: argument structures expanded field by field (fields left at zero are omitted), every pointer through
the caller's `ptr`, every other value through the caller's hooks."""
import contextlib
import ctypes as C

import torch


class _Recorder:
    def __init__(self, calls):
        self._calls = calls

    def __getattr__(self, name):
        def fn(*args):
            if self._calls is not None:
                self._calls.append((name, args))
            return 64 if name.endswith(("_bytes", "_elems")) else 0      # a size, so that every image has an address of its own
        return fn


def _req_dtype_only(t, dtype, name):
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    return t


@contextlib.contextmanager
def _seams(calls, made=None):
    """ops behind the three seams; `made` collects the tensors the call allocates (kept alive, so no address is used twice)"""
    from unimedvl_amd import _lib, ops
    saved = _lib.load, ops._stream, ops._req, torch.empty, torch.empty_like
    rec = _Recorder(calls)

    def keep(fn):
        def wrapped(*a, **kw):
            made.append(fn(*a, **kw))
            return made[-1]
        return wrapped
    _lib.load, ops._stream, ops._req = (lambda: rec), (lambda: None), _req_dtype_only
    if made is not None:
        torch.empty, torch.empty_like = keep(saved[3]), keep(saved[4])
    try:
        yield ops
    finally:
        _lib.load, ops._stream, ops._req, torch.empty, torch.empty_like = saved


def _struct(s, ptr, field):
    fields = []
    for f, ty in s._fields_:
        fv = getattr(s, f)
        if isinstance(fv, C.Structure):
            fields.append(f"{f}={_struct(fv, ptr, field)}")
        elif fv:
            fields.append(f"{f}={ptr(fv) if ty is C.c_void_p else field(f, fv)}")
    return "{" + " ".join(fields) + "}"


def render(calls, ptr, is_ptr=lambda v: False, field=lambda f, v: v, plain=lambda fn, i, v: str(v)):
    """["fn(arg, ...)", ...] of a log of (name, args).  ptr(v): the name of what the address v (an int, a c_void_p or None) points to;
    is_ptr(v): whether a plain integer argument is an address; field(name, v) / plain(fn, i, v): the text of a non-pointer structure
    field and of the i-th plain argument of fn"""
    items = []
    for name, args in calls:
        out = []
        for i, v in enumerate(args):
            if hasattr(v, "_obj"):          # byref(structure)
                out.append(_struct(v._obj, ptr, field))
            elif v is None or isinstance(v, C.c_void_p) or is_ptr(v):
                out.append(ptr(v))
            else:
                out.append(plain(name, i, v))
        items.append(f"{name}({', '.join(out)})")
    return items
