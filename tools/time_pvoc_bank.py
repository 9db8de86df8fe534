"""The filter bank of Pvoc (bank_kernels.hip: k_pvoc_bands) against the torch composition a caller writes without it:
(amp ** 2) @ W on a dense (M + 1) x B matrix built outside the timed region (and on a torch sparse W), then
.clamp_min(floor).log(), then @ D.T.  16 channels x 2^22 samples, hop = size / 4, the mel bank at B = 40 and 128.  Kernel
configurations: bands alone, POWER + LOG, POWER + LOG + DCT with 13 and with B coefficients, each against its torch
composition.  Three medians per leg, the legs interleaved in one process; the TB/s count the frames read once (the rows
written are B or ncoef floats per frame).  One JSON line per size and B, with the read figure of the same box
(bandwidth_probe) beside it, every ratio to torch — the cases the kernel loses included — the kernel's launches per call (one)
and the torch operators of each composition (a list of names, not a count of launches: an operator on the strided
frames[..., 0] may cost a copy besides).

    python tools/time_pvoc_bank.py [--sizes 256,2048,16384] [--bands 40,128] [--channels 16] [--log2-samples 22] [--reps 10]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import opencl_fft_amd as fa  # noqa: E402
from tools.time_pvoc import interleaved  # noqa: E402

FLOOR = 1e-10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,2048,16384")
    ap.add_argument("--bands", default="40,128")
    ap.add_argument("--channels", type=int, default=16)
    ap.add_argument("--log2-samples", type=int, default=22)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sr", type=float, default=48000.0)
    args = ap.parse_args()
    C, samples, sr = args.channels, 1 << args.log2_samples, args.sr
    dev = "cuda:0"
    read_tbs = fa.bandwidth_probe(0)["read"]
    for size in [int(s) for s in args.sizes.split(",")]:
        hop, M = size // 4, size // 2
        F = 1 + (samples - size) // hop
        g = torch.Generator(device=dev).manual_seed(size)
        a = torch.rand((C, F, M + 1, 2), device=dev, generator=g) + 0.01
        nbytes = a.numel() * 4
        for B in [int(s) for s in args.bands.split(",")]:
            pv = fa.Pvoc(0, size, hop, sr, C)
            assert pv.get_error() == 0, pv.get_log()
            first, count, weights = fa.Pvoc.mel_bank(size, sr, B)
            assert pv.bank_setup(first, count, weights) == 0
            W = np.zeros((M + 1, B), np.float32)
            off = 0
            for b in range(B):
                W[first[b]:first[b] + count[b], b] = weights[off:off + count[b]]
                off += count[b]
            W = torch.from_numpy(W).to(dev)
            Ws = W.to_sparse()
            D = torch.from_numpy(pv.bank_dct()).to(dev)
            outs = {n: torch.empty((C, F, n), device=dev) for n in {B, 13}}

            def mm(x, w):   # x: (C, F, M + 1), as frames[..., 0] gives it: strided, the caller's first operation
                return (x @ w) if w is W else torch.sparse.mm(w.t(), x.reshape(C * F, M + 1).t()).t()

            def t_bands(w=W):
                return mm(a[..., 0], w)

            def t_log(w=W):
                amp = a[..., 0]
                return mm(amp * amp, w).clamp_min(FLOOR).log()

            legs = {
                "bands": lambda: pv.bands_device(a, outs[B]),
                "torch_bands": t_bands,
                "torch_sparse_bands": lambda: t_bands(Ws),
                "power_log": lambda: pv.bands_device(a, outs[B], power=True, log=True, floor=FLOOR),
                "torch_power_log": t_log,
                "torch_sparse_power_log": lambda: t_log(Ws),
                "power_log_dct13": lambda: pv.bands_device(a, outs[13], power=True, log=True, ncoef=13, floor=FLOOR),
                "torch_power_log_dct13": lambda: t_log() @ D[:13].T,
                "power_log_dctB": lambda: pv.bands_device(a, outs[B], power=True, log=True, ncoef=B, floor=FLOOR),
                "torch_power_log_dctB": lambda: t_log() @ D.T,
            }
            for n in ("bands", "power_log", "power_log_dct13", "power_log_dctB"):
                assert legs[n]() == 0
            t = interleaved(legs, args.reps)
            med = {n: float(np.median(v)) for n, v in t.items()}
            ours = ("bands", "power_log", "power_log_dct13", "power_log_dctB")
            print(json.dumps({"size": size, "hop": hop, "channels": C, "frames": F, "bands": B, "bytes": nbytes,
                              "ms": {n: [round(u, 4) for u in v] for n, v in t.items()},
                              "tbs": {n: round(nbytes / med[n] / 1e9, 3) for n in ours},
                              "torch_over_kernel": dict(
                                  [(n, round(med["torch_" + n] / med[n], 2)) for n in ours] +
                                  [("sparse_" + n, round(med["torch_sparse_" + n] / med[n], 2)) for n in ours[:2]]),
                              "spread": {n: round((max(v) - min(v)) / med[n], 3) for n, v in t.items()},
                              "read_tbs": round(read_tbs, 3),
                              "kernel_launches": 1,
                              "torch_operators": {"torch_bands": ["mm"], "torch_power_log": ["mul", "mm", "clamp_min", "log"],
                                                  "torch_power_log_dct": ["mul", "mm", "clamp_min", "log", "mm"]},
                              "kernels": [pv.bands_kernel_name()]}), flush=True)
            del pv, W, Ws, D, outs
        del a
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
