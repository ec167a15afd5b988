"""The helpers the test modules share, each defined once: the text of csrc/, image formats and renders through the host and the
device entry, render options, and the environment switches of a case.  Data lives in tests/fixtures.py; this module needs no
built library, no torch and no GPU to import (torch is imported by the functions that use it)."""
import ctypes as C
import os
import re

import numpy as np

import fixtures as fx
import ntracer_amd
from ntracer_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ntracer_amd", "csrc")


# ---- source text

def source(name):
    """a file of ntracer_amd/csrc/ as text"""
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def function_body(src, head):
    """the text of the function that starts with `head`, up to its closing brace in column 0"""
    start = src.index(head)
    return src[start:re.compile(r"\n\}(\n|$)").search(src, start).start()]


def launches(body):
    """instantiations launched in `body`, spaces dropped: `hipLaunchKernelGGL((name<...>), ...` or `hipLaunchKernelGGL(name, ...`"""
    names = re.findall(r"hipLaunchKernelGGL\(\s*\(?\s*([A-Za-z_]\w*(?:\s*<[^<>]*>)?)", body)
    return {re.sub(r"\s+", "", n) for n in names}


# the helpers of the fixed-n launchers' shared set-up (nt_composite.hpp) that launch a kernel themselves
SHARED_LAUNCHERS = ("packet_chunk_head",)


def launches_through(src, head):
    """launches() of the function that starts with `head`, and of every shared helper that its body calls"""
    body = function_body(src, head)
    names = launches(body)
    for helper in SHARED_LAUNCHERS:
        if re.search(r"\b%s\s*(<[^<>;()]*>)?\s*\(" % helper, body):
            names |= launches(function_body(source("nt_composite.hpp"), "int %s(" % helper))
    return names


# ---- formats and renders

def fmt_of(w, h, chans=fx.RGBX8, pitch=0, rev=False):
    return ntracer_amd.ImageFormat(w, h, [ntracer_amd.Channel(*c) for c in chans], pitch, rev)


def render_host(scene, fmt, fill=0, **kw):
    """(height, pitch) uint8 through BlockingRenderer, over a buffer of `fill` bytes"""
    buf = bytearray(bytes([fill]) * (fmt.pitch * fmt.height))
    assert ntracer_amd.BlockingRenderer().render(buf, fmt, scene, **kw)
    return np.frombuffer(bytes(buf), np.uint8).reshape(fmt.height, fmt.pitch)


def render_device(sc, fmt, opts=None, fill=0x3D):
    """(status, rows) of nt_render_device into a device buffer with 16 guard bytes behind it, which must come back untouched"""
    import torch
    size = fmt.pitch * fmt.height
    buf = torch.full((size + 16,), fill, dtype=torch.uint8, device="cuda")
    fst = fmt._as_struct()
    status = _lib.lib().nt_render_device(sc._handle, C.c_void_p(buf.data_ptr()), size, C.byref(fst), None if opts is None else C.byref(opts),
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[size:] == fill).all()
    return status, got[:size].reshape(fmt.height, fmt.pitch)


def render_opts(abort=None, **fields):
    """an NtRenderOpts on the current device, with `fields` set and `abort` (a device tensor) as its abort word"""
    opts = _lib.NtRenderOpts()
    opts.device = -1
    for k, v in fields.items():
        setattr(opts, k, v)
    if abort is not None:
        opts.abort_device = abort.data_ptr()
    return opts


def strict_reference():
    """NtRenderOpts.strict_reference as NTRACER_STRICT_REFERENCE asks for it now"""
    return 1 if os.environ.get("NTRACER_STRICT_REFERENCE", "0") not in ("", "0") else 0


def cuda_device():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def worker_threads():
    """threads for an oracle render: the cores this process may use, less one"""
    import bench
    return max(1, min(64, bench.cpu_quota_cores() - 1))


# ---- switches

def set_switches(mp, names, env):
    """every switch of `names` cleared, then those of `env` set, through the monkeypatch `mp`"""
    for k in names:
        mp.delenv(k, raising=False)
    for k, v in env.items():
        mp.setenv(k, v)
