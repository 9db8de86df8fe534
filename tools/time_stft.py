"""Fused short-time analysis / synthesis (Stft, stft_kernels.hip) against the composition a caller writes today:
analysis = as_strided framing times the window in one torch op, then Clrfft.exec_device; synthesis = Clrfft inverse
(exec_device_oop), the window, torch.nn.functional.fold.  16 channels x 2^22 samples, hop = size / 4.  Prints one JSON
line per size; algorithmic TB/s counts signal bytes + spectra bytes once.  The host legs time the blocking forms
(clfa_stft_analyze / clfa_stft_synthesize on host arrays, copies included) on 2 channels x 2^--host-log2-samples samples.

    python tools/time_stft.py [--sizes 256,1024,2048,4096,16384] [--channels 16] [--log2-samples 22] [--reps 20]
                              [--host-log2-samples 16] [--host-reps 50]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as Fn  # noqa: E402

import opencl_fft_amd as fa  # noqa: E402
from opencl_fft_amd import _lib  # noqa: E402


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))   # ms


def timed_host(fn, reps, warm=3):
    for _ in range(warm):
        assert fn() == 0
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3   # ms


def host_legs(an, sy, size, samples, reps):
    """the blocking forms on 2 padded rows of `samples` floats (row stride samples + 3)"""
    L = _lib.lib()
    F = an.frames(samples)
    n = sy.samples(F)
    x = np.random.default_rng(size).random((2, samples + 3), dtype=np.float32) * 2 - 1
    spec = np.zeros((2, F, size // 2), np.complex64)
    y = np.zeros((2, n + 3), np.float32)
    t_an = timed_host(lambda: L.clfa_stft_analyze(an._h, x.ctypes.data, samples + 3, samples, 2, spec.ctypes.data), reps)
    t_sy = timed_host(lambda: L.clfa_stft_synthesize(sy._h, spec.ctypes.data, F, 2, y.ctypes.data, n + 3, 0), reps)
    return t_an, t_sy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,1024,2048,4096,16384")
    ap.add_argument("--channels", type=int, default=16)
    ap.add_argument("--log2-samples", type=int, default=22)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-log2-samples", type=int, default=16)
    ap.add_argument("--host-reps", type=int, default=50)
    args = ap.parse_args()
    C, samples = args.channels, 1 << args.log2_samples
    dev = "cuda:0"
    x = torch.rand((C, samples), device=dev) * 2 - 1
    for size in [int(s) for s in args.sizes.split(",")]:
        hop, M = size // 4, size // 2
        w = torch.from_numpy((0.5 - 0.5 * np.cos(2 * np.pi * np.arange(size) / size)).astype(np.float32)).to(dev)
        an, sy = fa.Stft(0, size, hop, window=w), fa.Stft(0, size, hop, window=w, fwd=False)
        assert an.get_error() == 0 and sy.get_error() == 0
        F = an.frames(samples)
        L = sy.samples(F)
        spec = torch.empty((C, F, M), dtype=torch.complex64, device=dev)
        y = torch.empty((C, L), device=dev)
        t_an = timed(lambda: an.analyze_device(x, spec), args.reps)
        t_sy = timed(lambda: sy.synthesize_device(spec, y, normalize=False), args.reps)
        t_han, t_hsy = host_legs(an, sy, size, max(1 << args.host_log2_samples, size), args.host_reps)
        # the composition
        fwd, inv = fa.Clrfft(0, size, True), fa.Clrfft(0, size, False)
        frames = torch.empty((C, F, size), device=dev)
        xv = x.as_strided((C, F, size), (samples, hop, 1))

        def comp_an():
            torch.mul(xv, w, out=frames)
            assert fwd.exec_device(frames, C * F) == 0

        r = torch.empty((C, F, size), device=dev)

        def comp_sy():
            assert inv.exec_device_oop(spec, r, C * F) == 0
            rw = r * w
            Fn.fold(rw.transpose(1, 2), output_size=(1, L), kernel_size=(1, size), stride=(1, hop))

        t_can = timed(comp_an, args.reps)
        t_csy = timed(comp_sy, args.reps)
        bytes_ = C * samples * 4 + C * F * M * 8
        bytes_sy = C * L * 4 + C * F * M * 8
        print(json.dumps({"size": size, "hop": hop, "channels": C, "samples": samples, "frames": F,
                          "analyze_ms": round(t_an, 4), "analyze_tbs": round(bytes_ / t_an / 1e9, 3),
                          "compose_analyze_ms": round(t_can, 4), "analyze_speedup": round(t_can / t_an, 2),
                          "synth_ms": round(t_sy, 4), "synth_tbs": round(bytes_sy / t_sy / 1e9, 3),
                          "compose_synth_ms": round(t_csy, 4), "synth_speedup": round(t_csy / t_sy, 2),
                          "host_analyze_ms": round(t_han, 4), "host_synth_ms": round(t_hsy, 4)}), flush=True)
        del frames, r, spec, y
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
