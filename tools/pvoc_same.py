#!/usr/bin/env python3
"""Bits of Pvoc's C ABI, for comparing two builds of the library: a fixed, seeded call sequence over every family of calls
in both forms, one line per call with the return code, a sha256 over every output's bytes and the object's counters, and
after each stateful call a sha256 of every readable state.  Run it once per build, each in a process of its own, and
compare the printouts: `python tools/pvoc_same.py --lib PATH > a.txt`.

Objects: size 64 / hop 16 / 2 channels, and size 1024 / hop 256 / 1 channel (M = 512: the 256-lane group kernels of desc,
trace and pitch take several passes), each once plain and once under CLFA_PVOC_CHUNKS_MAX=1, CLFA_PVOC_OPS_GRID_MAX=2 and
CLFA_PVOC_ADSYN_GRID_MAX=2 (several sub-batches, wrapped grids).  The stream is cut into calls of 1, 3 and 130 frames.
--time: us per call of the F = 1 device and blocking forms of mix, smooth, bands and pitch at size 64 / 1 channel."""
import argparse
import ctypes as C
import hashlib
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opencl_fft_amd import _lib  # noqa: E402
from opencl_fft_amd.pvoc import Pvoc  # noqa: E402

RNG = np.random.RandomState(20250117)
SR = 48000.0
f32 = np.float32
SWITCHES = {"CLFA_PVOC_CHUNKS_MAX": "1", "CLFA_PVOC_OPS_GRID_MAX": "2", "CLFA_PVOC_ADSYN_GRID_MAX": "2"}
COUNTERS = ("workspace_bytes", "adsyn_workspace_bytes", "time_state_bytes", "delay_state_bytes", "desc_state_bytes",
            "bank_state_bytes", "blur_max_frames", "delay_max_frames", "bank_bands")


def bind(path):
    lib = C.CDLL(path)
    for name, res, args in _lib.SYMBOLS:
        f = getattr(lib, name)
        f.restype, f.argtypes = res, args
    return lib


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


class Form:
    """the arrays of one call in one form: host arrays for the blocking form, device tensors for the device form"""

    def __init__(self, dev):
        self.dev, self.keep, self.outs = dev, [], []

    def ptr(self, a, offset=0):
        if a is None:
            return None
        a = torch.from_numpy(np.ascontiguousarray(a)).cuda() if self.dev else np.ascontiguousarray(a)
        self.keep.append(a)
        return (a.data_ptr() if self.dev else a.ctypes.data) + offset

    def out(self, shape, dtype=f32):
        p = self.ptr(np.zeros(shape, dtype))
        self.outs.append(self.keep[-1])
        return p

    def tail(self):
        return (torch.cuda.current_stream().cuda_stream,) if self.dev else ()

    def digest(self):
        torch.cuda.synchronize()
        return " ".join(sha(o.cpu().numpy() if self.dev else o) for o in self.outs) or "-"


class Obj:
    def __init__(self, lib, size, hop, ch, tag):
        self.lib, self.size, self.hop, self.ch, self.M, self.tag = lib, size, hop, ch, size // 2, tag
        self.p = C.c_void_p()
        rc = lib.clfa_pvoc_create(C.byref(self.p), 0, size, hop, SR, ch)
        self.line("create", rc, "-")

    def f(self, name):
        return getattr(self.lib, "clfa_pvoc_" + name)

    def line(self, what, rc, digest):
        print("%-44s rc %5d  %s  | %s" % (self.tag + " " + what, rc, digest, " ".join(str(self.f(c)(self.p)) for c in COUNTERS)))

    def states(self, what):
        """every readable state: return code and sha256"""
        n, got = self.ch * (self.M + 1), []

        def read(name, shape, dtype, *args):
            a = np.zeros(shape, dtype)
            got.append("%s:%d:%s" % (name, self.f(name)(self.p, *args, a.ctypes.data), sha(a)))
        read("read_phase", n, np.uint32)
        read("read_prev", n, np.complex64)
        P, W, A = np.zeros(n, np.uint64), np.zeros(n, np.int32), np.zeros(n, f32)
        got.append("adsyn:%d:%s" % (self.f("adsyn_read_state")(self.p, P.ctypes.data, W.ctypes.data, A.ctypes.data), sha(P) + sha(W) + sha(A)))
        for op in range(3):
            rows = max(self.f("blur_max_frames")(self.p) - 1, 0) if op == 0 else 1
            read("time_read_state", (rows, n, 2), f32, op)
        for which in range(2):
            read("delay_read_state", (max(self.f("delay_max_frames")(self.p), 0), n, 2), f32, which)
        read("desc_read_state", n, f32)
        B = max(self.f("bank_bands")(self.p), 0)
        read("bank_read_dct", (B, B), f32)
        print("%-44s %s" % (self.tag + " " + what + " states", " ".join(got)))

    def frames(self, F):
        amp = RNG.rand(self.ch, F, self.M + 1).astype(f32) ** 4
        freq = ((np.arange(self.M + 1) + RNG.rand(self.ch, F, self.M + 1) - 0.5) * SR / self.size).astype(f32)
        return np.stack([amp, freq], axis=-1)

    def call(self, what, name, dev, build, stateful=False):
        """build(form) -> the arguments after the object; the form's tail (the stream) follows them"""
        fm = Form(dev)
        rc = self.f(name + ("_dev" if dev else ""))(self.p, *build(fm), *fm.tail())
        self.line("%s %s" % (what, "dev" if dev else "host"), rc, fm.digest())
        if stateful:
            self.states(what)

    def families(self, F, dev):
        ch, M, fshape, t = self.ch, self.M, (self.ch, F, self.M + 1, 2), "F%d " % F
        spec = (RNG.rand(ch, F, M, 2).astype(f32) - 0.5).view(np.complex64)
        self.call(t + "analyze", "analyze", dev, lambda m: (m.ptr(spec), m.out(fshape), F), True)
        self.call(t + "synthesize", "synthesize", dev, lambda m: (m.ptr(self.frames(F)), m.out((ch, F, M), np.complex64), F), True)
        for keep in (0, 1):
            scale, shift = (0.5 + 1.5 * RNG.rand(F)).astype(f32), (2000 * RNG.rand(F) - 1000).astype(f32)
            self.call(t + "scale keepform %d" % keep, "scale", dev, lambda m: (m.ptr(self.frames(F)), m.out(fshape), F, m.ptr(scale), keep, 0.9, 8))
            self.call(t + "shift keepform %d" % keep, "shift", dev, lambda m: (m.ptr(self.frames(F)), m.out(fshape), F, m.ptr(shift), 2, keep, 0.9, 8))
        pos = (RNG.rand(F + 2) * (F - 1)).astype(f32)
        self.call(t + "read", "read", dev, lambda m: (m.ptr(self.frames(F)), F, m.ptr(pos), m.out((ch, F + 2, M + 1, 2)), F + 2))
        for op in range(5):
            pq = RNG.rand(2, F).astype(f32)
            self.call(t + "pair %d" % op, "pair", dev, lambda m: (op, m.ptr(self.frames(F)), m.ptr(self.frames(F)), m.out(fshape), F,
                                                                 m.ptr(pq[0]), m.ptr(pq[1]), 8))
        for op in range(6):
            par = RNG.rand(F, 4).astype(f32)
            if op == 0:
                par = np.sort(par, axis=1) * f32(SR / 2)
            if op == 5:
                par[:, 0] += 0.5
            table = RNG.rand(M + 1).astype(f32) if op in (1, 2) else None
            self.call(t + "shape %d" % op, "shape", dev, lambda m: (op, m.ptr(self.frames(F)), m.out(fshape), F, m.ptr(par), m.ptr(table),
                                                                   int(op == 0), 2, 8))
        blur = max(self.f("blur_max_frames")(self.p), 1)
        for op in range(3):
            p = np.floor(1 + RNG.rand(F) * blur).astype(f32) if op == 0 else RNG.rand(F).astype(f32)
            q = None if op == 0 else (RNG.rand(F).astype(f32) if op == 1 else (RNG.rand(F) > 0.5).astype(f32))
            p = (p > 0.5).astype(f32) if op == 2 else p
            self.call(t + "time %d" % op, "time", dev, lambda m: (op, m.ptr(self.frames(F)), m.out(fshape), F, m.ptr(p), m.ptr(q)), True)
        L = self.f("delay_max_frames")(self.p)
        for fb in (False, True):
            d = RNG.randint(0, max(L, 0) + 1, M + 1).astype(np.int32)
            g = (1.6 * RNG.rand(M + 1) - 0.8).astype(f32) if fb else None
            self.call(t + "delay L %d fb %d" % (L, fb), "delay", dev, lambda m: (m.ptr(self.frames(F)), m.out(fshape), F, m.ptr(d), m.ptr(g)), True)
        for rect in (0, 1):
            self.call(t + "desc rectify %d" % rect, "desc", dev, lambda m: (m.ptr(self.frames(F)), m.out((ch, F, 8)), F, 1, M - 1, rect), True)
        B = max(self.f("bank_bands")(self.p), 1)
        for flags, ncoef in ((0, 0), (1, 0), (2, 0), (7, 5)):
            self.call(t + "bands flags %d" % flags, "bands", dev, lambda m: (m.ptr(self.frames(F)), m.out((ch, F, ncoef or B)), F, flags, ncoef, 1e-6))
        n = (RNG.rand(F) * 10).astype(f32)
        self.call(t + "trace", "trace", dev, lambda m: (m.ptr(self.frames(F)), m.out(fshape), m.ptr(n), None, 0, F, 0, M + 1, 0))
        self.call(t + "trace list residual", "trace", dev, lambda m: (m.ptr(self.frames(F)), m.out(fshape), m.ptr(n), m.out((ch, F, 4), np.int32), 4, F, 1, M - 1, 1))
        par = np.stack([2 * RNG.rand(F) - 1, 1 + 10 * RNG.rand(F)], axis=1).astype(f32)
        self.call(t + "demix", "demix", dev, lambda m: (m.ptr(self.frames(F)), m.ptr(self.frames(F)), m.out(fshape), m.ptr(par), None, F, 5, 0, M + 1))
        self.call(t + "demix az", "demix", dev, lambda m: (m.ptr(self.frames(F)), m.ptr(self.frames(F)), m.out(fshape), m.ptr(par), m.out((ch, F, 11)), F, 5, 1, M - 1))
        self.call(t + "pitch", "pitch", dev, lambda m: (m.ptr(self.frames(F)), m.out((ch, F, 4)), None, F, 1, M - 1, 8, 0.05, 50.0, SR / 4, 0.03, 0.84))
        self.call(t + "pitch peaks", "pitch", dev, lambda m: (m.ptr(self.frames(F)), m.out((ch, F, 4)), m.out((ch, F, 8, 2)), F, 2, M - 3, 8, 0.05, 50.0, SR / 4, 0.03, 0.84))
        samples, window = 5 * self.size + 3, (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(self.size) / self.size)).astype(f32)
        signal, starts = RNG.rand(ch, samples + 5).astype(f32) - 0.5, RNG.randint(-self.size, samples, F).astype(np.int32)
        self.call(t + "tanal strided", "tanal", dev, lambda m: (m.ptr(signal), samples + 5, samples, m.ptr(window), m.ptr(starts), m.out(fshape), F))
        for fmod in (None, (0.5 + RNG.rand(F)).astype(f32)):
            self.call(t + "adsyn strided fmod %d" % (fmod is not None), "adsyn", dev,
                      lambda m: (m.ptr(self.frames(F)), F, m.ptr(fmod), 1, (M - 1) // 2, 2, 0.1, m.out((ch, F * self.hop + 5)), F * self.hop + 5), True)

    def refused(self, dev):
        """NULL, misaligned (device form), an output overlapping an input, F = 0, F < 0"""
        M, F = self.M, 2
        fshape, par = (self.ch, F, M + 1, 2), np.ones(F, f32)
        self.call("refused NULL in", "scale", dev, lambda m: (None, m.out(fshape), F, m.ptr(par), 0, 1.0, 8))
        self.call("refused NULL out", "desc", dev, lambda m: (m.ptr(self.frames(F)), None, F, 0, M + 1, 0))
        self.call("misaligned in", "scale", dev, lambda m: (m.ptr(np.zeros(self.ch * F * (M + 1) * 2 + 1, f32), 4), m.out(fshape), F, m.ptr(par), 0, 1.0, 8))
        def overlap(m):
            o = m.out(fshape)
            return (o, o, F, m.ptr(par), 0, 1.0, 8)
        self.call("refused overlap", "scale", dev, overlap)
        for n in (0, -1):
            self.call("F %d" % n, "scale", dev, lambda m: (m.ptr(self.frames(F)), m.out(fshape), n, m.ptr(par), 0, 1.0, 8))
            self.call("F %d" % n, "pitch", dev, lambda m: (m.ptr(self.frames(F)), m.out((self.ch, F, 4)), None, n, 1, M - 1, 8, 0.05, 50.0, SR / 4, 0.03, 0.84))

    def setup(self, name, *args):
        self.line("%s%s" % (name, args[:1]), self.f(name)(self.p, *args), "-")
        self.states(name)

    def run(self):
        for dev in (True, False):                 # before the set-ups: blur, delay and bands are refused
            self.families(1, dev)
            self.refused(dev)
        self.setup("blur_setup", 4)
        self.setup("delay_setup", 3)
        first, count, weights = Pvoc.mel_bank(self.size, SR, 8)
        self.setup("bank_setup", 8, first.ctypes.data, count.ctypes.data, weights.ctypes.data)
        for F in (1, 3, 130):
            for dev in (True, False):
                self.families(F, dev)
            if F == 3:
                self.setup("reset")
        self.setup("delay_setup", 5)
        self.setup("blur_setup", 0)               # refused: the object stays as it was
        for dev in (True, False):
            self.families(3, dev)
        self.f("destroy")(self.p)


def timing(lib, calls, warm):
    size, M, s = 64, 32, torch.cuda.current_stream().cuda_stream
    p = C.c_void_p()
    assert lib.clfa_pvoc_create(C.byref(p), 0, size, 16, SR, 1) == 0
    first, count, weights = Pvoc.mel_bank(size, SR, 8)
    assert lib.clfa_pvoc_bank_setup(p, 8, first.ctypes.data, count.ctypes.data, weights.ctypes.data) == 0
    fr = np.stack([RNG.rand(1, 1, M + 1), RNG.rand(1, 1, M + 1) * SR / 2], axis=-1).astype(f32)
    half, out, rows = f32([0.5]), np.zeros((1, 1, M + 1, 2), f32), np.zeros((1, 1, 8), f32)
    d = {k: torch.from_numpy(v).cuda() for k, v in dict(fr=fr, half=half, out=out, rows=rows).items()}
    host = {k: v.ctypes.data for k, v in dict(fr=fr, half=half, out=out, rows=rows).items()}
    dev = {k: v.data_ptr() for k, v in d.items()}
    for form, a, tail in (("dev", dev, (s,)), ("host", host, ())):
        sfx = "_dev" if form == "dev" else ""
        rows_ = {"mix": lambda: getattr(lib, "clfa_pvoc_pair" + sfx)(p, 3, a["fr"], a["fr"], a["out"], 1, None, None, 1, *tail),
                 "smooth": lambda: getattr(lib, "clfa_pvoc_time" + sfx)(p, 1, a["fr"], a["out"], 1, a["half"], a["half"], *tail),
                 "bands": lambda: getattr(lib, "clfa_pvoc_bands" + sfx)(p, a["fr"], a["rows"], 1, 0, 0, 1e-6, *tail),
                 "pitch": lambda: getattr(lib, "clfa_pvoc_pitch" + sfx)(p, a["fr"], a["rows"], None, 1, 1, M - 1, 8, 0.05, 50.0, SR / 4, 0.03, 0.84, *tail)}
        for name, call in rows_.items():
            for _ in range(warm):
                assert call() == 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                call()
            torch.cuda.synchronize()
            print("%-8s %-5s F 1  %8.2f us per call (%d calls)" % (name, form, (time.perf_counter() - t0) / calls * 1e6, calls))
    lib.clfa_pvoc_destroy(p)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lib", required=True, help="the libclfft_amd.so to run")
    ap.add_argument("--time", action="store_true", help="time the F = 1 forms of mix, smooth, bands and pitch instead")
    ap.add_argument("--calls", type=int, default=4000)
    args = ap.parse_args()
    lib = bind(args.lib)
    torch.zeros(1, device="cuda")
    if args.time:
        return timing(lib, args.calls, 500)
    for size, hop, ch in ((64, 16, 2), (1024, 256, 1)):
        for switches in ({}, SWITCHES):
            os.environ.update(switches)
            o = Obj(lib, size, hop, ch, "%d/%d/%d%s" % (size, hop, ch, " sw" if switches else ""))
            for k in switches:
                del os.environ[k]
            o.run()


if __name__ == "__main__":
    main()
