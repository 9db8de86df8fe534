#!/usr/bin/env python3
"""Bits of the convolutions' C ABI, for comparing two builds of the library: a fixed, seeded call sequence over all five
convolution objects at the smallest shapes that reach every branch of the host layer, one line per call with the return
code, a sha256 over the output bytes, and the object's position / byte counters.  Run it once per build, each in a
process of its own, and compare the printouts: `python tools/conv_same.py --lib PATH > a.txt`.

Non-uniform objects: pts0 32, pts1 128, cvs 640 (m = 4, head 8 partitions, tail 3, response period 20 head blocks), 3
channels / 3 inputs x 2 outputs, the matrix a second time with CLFA_PCONV_MATRIX_SEGS=3."""
import argparse
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opencl_fft_amd import _lib  # noqa: E402

RNG = np.random.RandomState(20240521)


def bind(path):
    lib = C.CDLL(path)
    for name, res, args in _lib.SYMBOLS:
        f = getattr(lib, name)
        f.restype, f.argtypes = res, args
    return lib


def rows(r, n):
    return (RNG.rand(r, n).astype(np.float32) - 0.5)


def dev(a):
    return torch.from_numpy(a).cuda()


def line(tag, rc, out, *counters):
    torch.cuda.synchronize()
    data = out.cpu().numpy().tobytes() if isinstance(out, torch.Tensor) else (out.tobytes() if out is not None else b"")
    print("%-34s rc %5d  %s  %s" % (tag, rc, hashlib.sha256(data).hexdigest()[:24], " ".join(str(c) for c in counters)))


def nup(lib, kind, rin, rout, tag):
    """kind: 'nupconv' (rin channels) or 'nupconv_matrix' (rin inputs, rout outputs)"""
    f = lambda name: getattr(lib, "clfa_%s_%s" % (kind, name))
    tv, cvs, pts0 = kind == "nupconv", 640, 32
    p = C.c_void_p()
    rc = f("create")(C.byref(p), 0, cvs, pts0, 128, *((rin,) if tv else (rin, rout)))
    rresp, s = (rin if tv else rin * rout), torch.cuda.current_stream().cuda_stream
    count = lambda: (f("position")(p), f("state_bytes")(p), f("workspace_bytes")(p), f("fade_remaining")(p))
    line(tag + " create", rc, None, *count())

    def proc(n, name="process_dev", second=False):
        x, o = dev(rows(rin, n * pts0)), torch.zeros((rout, n * pts0), device="cuda")
        if second:
            x2 = dev(rows(rin, n * pts0))
            rc = f("process_tv_dev")(p, o.data_ptr(), n * pts0, x.data_ptr(), n * pts0, x2.data_ptr(), n * pts0, n, s)
        else:
            rc = f("process_dev")(p, o.data_ptr(), n * pts0, x.data_ptr(), n * pts0, n, s)
        line("%s %s%s %d" % (tag, name, " tv" if second else "", n), rc, o, *count())

    def push(fade=0, stride=cvs):
        h = dev(rows(rresp, cvs))
        rc = f("push_ir_fade_dev")(p, h.data_ptr(), stride, fade, s) if fade else f("push_ir_dev")(p, h.data_ptr(), stride, s)
        line("%s push fade %d stride %d" % (tag, fade, stride), rc, None, *count())

    push()
    for _ in range(14):
        proc(1)
    proc(7)
    push(fade=5)                      # at phase 1 of its period
    proc(8)                           # the fade's 5 blocks and 3 on the usual route
    push(fade=3)
    for _ in range(4):                # the fade block by block, and one block after it
        proc(1)
    if tv:                            # position 33 = 13 in the response period of 20: 23 blocks cross its end and a = n0
        for n in (1, 3, 23):
            proc(n, second=True)
    push(stride=cvs - 1)              # refused: rows too short
    push(fade=4)
    push()                            # refused: a fade is pending
    if tv:
        proc(2, second=True)          # refused as well
    line(tag + " reset in fade", f("reset")(p, s), None, *count())
    proc(4)
    line(tag + " reset", f("reset")(p, s), None, *count())
    push()
    proc(1)
    proc(5)
    # the blocking host forms
    h, x, o = rows(rresp, cvs), rows(rin, 3 * pts0), np.zeros((rout, 3 * pts0), np.float32)
    line(tag + " push_ir", f("push_ir")(p, h.ctypes.data), None, *count())
    line(tag + " convolution", f("convolution")(p, o.ctypes.data, x.ctypes.data, 3), o, *count())
    line(tag + " push_ir_fade", f("push_ir_fade")(p, h.ctypes.data, 2), None, *count())
    line(tag + " convolution", f("convolution")(p, o.ctypes.data, x.ctypes.data, 3), o, *count())
    if tv:
        x2 = rows(rin, 3 * pts0)
        line(tag + " convolution_tv", f("convolution_tv")(p, o.ctypes.data, x.ctypes.data, x2.ctypes.data, 3), o, *count())
    f("destroy")(p)


def blocks(lib, kind, create_args, ch, pts, irlen, tag):
    """Clpconv / Cldconv: single blocks and the blocks route with one and two inputs, device and blocking forms"""
    f = lambda name: getattr(lib, "clfa_%s_%s" % (kind, name))
    p, s = C.c_void_p(), torch.cuda.current_stream().cuda_stream
    rc = f("create_channels" if kind == "dconv" else "create")(C.byref(p), 0, *create_args)
    line(tag + " create", rc, None, f("state_bytes")(p))
    h = dev(rows(ch, irlen))
    line(tag + " push_ir_dev", f("push_ir_dev")(p, h.data_ptr(), irlen, s), None)
    for two in (False, True):
        for n in (1, 1, 5):
            x, x2, o = dev(rows(ch, n * pts)), dev(rows(ch, n * pts)), torch.zeros((ch, n * pts), device="cuda")
            b = x2.data_ptr() if two else None
            rc = (f("process_dev")(p, o.data_ptr(), x.data_ptr(), b, s) if n == 1 else
                  f("process_blocks_dev")(p, o.data_ptr(), n * pts, x.data_ptr(), b, n * pts, n, s))
            line("%s dev %d inputs %d" % (tag, n, 1 + two), rc, o, f("wp")(p), f("blocks_workspace_bytes")(p))
    hh, x, x2, o = rows(ch, irlen), rows(ch, 5 * pts), rows(ch, 5 * pts), np.zeros((ch, 5 * pts), np.float32)
    line(tag + " push_ir", f("push_ir")(p, hh.ctypes.data), None)
    line(tag + " convolution", f("convolution")(p, o.ctypes.data, x.ctypes.data), o[:, :pts] if ch == 1 else o.reshape(-1)[:ch * pts], f("wp")(p))
    line(tag + " convolution_tv", f("convolution_tv")(p, o.ctypes.data, x.ctypes.data, x2.ctypes.data), o.reshape(-1)[:ch * pts], f("wp")(p))
    for b in (None, x2.ctypes.data):
        line(tag + " convolution_blocks", f("convolution_blocks")(p, o.ctypes.data, x.ctypes.data, b, 5), o, f("wp")(p))
    f("destroy")(p)


def matrix(lib, tag):
    f = lambda name: getattr(lib, "clfa_pconv_matrix_" + name)
    p, s, pts = C.c_void_p(), torch.cuda.current_stream().cuda_stream, 32
    line(tag + " create", f("create")(C.byref(p), 0, 128, pts, 3, 2), None)
    count = lambda: (f("state_bytes")(p), f("workspace_bytes")(p), f("fade_remaining")(p))
    for fade in (0, 3):
        h = dev(rows(6, 128))
        rc = f("push_ir_fade_dev")(p, h.data_ptr(), 128, fade, s) if fade else f("push_ir_dev")(p, h.data_ptr(), 128, s)
        line("%s push fade %d" % (tag, fade), rc, None, *count())
        x, o = dev(rows(3, 5 * pts)), torch.zeros((2, 5 * pts), device="cuda")
        line(tag + " process_dev 5", f("process_dev")(p, o.data_ptr(), 5 * pts, x.data_ptr(), 5 * pts, 5, s), o, *count())
    h, x, o = rows(6, 128), rows(3, 5 * pts), np.zeros((2, 5 * pts), np.float32)
    line(tag + " push_ir_fade", f("push_ir_fade")(p, h.ctypes.data, 2), None, *count())
    line(tag + " convolution", f("convolution")(p, o.ctypes.data, x.ctypes.data, 5), o, *count())
    f("destroy")(p)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lib", required=True, help="the libclfft_amd.so to run")
    lib = bind(ap.parse_args().lib)
    torch.zeros(1, device="cuda")
    nup(lib, "nupconv", 3, 3, "nupconv")
    nup(lib, "nupconv_matrix", 3, 2, "nupm")
    os.environ["CLFA_PCONV_MATRIX_SEGS"] = "3"
    nup(lib, "nupconv_matrix", 3, 2, "nupm segs3")
    del os.environ["CLFA_PCONV_MATRIX_SEGS"]
    blocks(lib, "pconv", (128, 32, 3), 3, 32, 128, "pconv")
    for ch in (1, 2):
        blocks(lib, "dconv", (40, 16, ch), ch, 16, 40, "dconv ch%d" % ch)
    matrix(lib, "pconv_matrix")


if __name__ == "__main__":
    main()
