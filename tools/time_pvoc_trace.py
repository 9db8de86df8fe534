"""The N loudest bins of Pvoc (pvoc_trace.hip: k_pvoc_trace) against the torch composition a caller writes without it:
torch.topk on the amps, a scatter of the values into zeros and a stack with the freq column.  16 channels x 2^22
samples, hop = size / 4, N = 8, M / 8 and M / 2.  Three medians per leg, the legs interleaved; algorithmic GB/s counts one
stream in and one out.  A further leg writes the bin list (N entries per frame) as well.  One JSON line per size and N,
with the copy figure of the same box (bandwidth_probe) beside it: the kernel reads a stream and writes one.

    python tools/time_pvoc_trace.py [--sizes 256,2048,16384] [--channels 16] [--log2-samples 22] [--reps 10]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,2048,16384")
    ap.add_argument("--channels", type=int, default=16)
    ap.add_argument("--log2-samples", type=int, default=22)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sr", type=float, default=48000.0)
    args = ap.parse_args()
    C, samples, sr = args.channels, 1 << args.log2_samples, args.sr
    dev = "cuda:0"
    copy_tbs = fa.bandwidth_probe(0)["copy"]
    for size in [int(s) for s in args.sizes.split(",")]:
        hop, M = size // 4, size // 2
        pv = fa.Pvoc(0, size, hop, sr, C)
        assert pv.get_error() == 0, pv.get_log()
        F = 1 + (samples - size) // hop
        g = torch.Generator(device=dev).manual_seed(size)
        a = torch.rand((C, F, M + 1, 2), device=dev, generator=g) + 0.01
        a[..., 1] = (a[..., 1] - 0.51 + torch.arange(M + 1, device=dev)) * (sr / size)      # freqs around the bin centres
        out = torch.empty_like(a)
        for N in (8, M // 8, M // 2):
            n = torch.full((F,), float(N), device=dev)
            lst = torch.empty((C, F, N), dtype=torch.int32, device=dev)

            def compose():
                amp = a[..., 0]
                top, idx = torch.topk(amp, N, dim=-1)
                return torch.stack([torch.zeros_like(amp).scatter_(-1, idx, top), a[..., 1]], dim=-1)

            legs = {"trace": lambda: pv.trace_device(a, out, n), "compose_trace": compose,
                    "trace_list": lambda: pv.trace_device(a, out, n, bins_out=lst),
                    "residual": lambda: pv.trace_device(a, out, n, residual=True)}
            assert legs["trace"]() == 0 and legs["trace_list"]() == 0 and legs["residual"]() == 0
            # the two agree where the amps are distinct (random floats: ties are rare and broken alike, lower bin first or not)
            assert pv.trace_device(a, out, n) == 0
            kept = int((out[0, :64, :, 0] != 0).sum())
            assert kept == 64 * N, kept
            t = interleaved(legs, args.reps)
            med = {k: float(np.median(v)) for k, v in t.items()}
            nbytes = 2 * a.numel() * 4
            print(json.dumps({"size": size, "hop": hop, "channels": C, "frames": F, "N": N, "bytes": nbytes,
                              "ms": {k: [round(u, 4) for u in v] for k, v in t.items()},
                              "gbs": {k: round(nbytes / med[k] / 1e6, 1) for k in legs},
                              "ratio": {"compose_over_trace": round(med["compose_trace"] / med["trace"], 2)},
                              "spread": {k: round((max(v) - min(v)) / med[k], 3) for k, v in t.items()},
                              "copy_gbs": round(copy_tbs * 1e3, 1),
                              "kernels": [pv.trace_kernel_name()]}), flush=True)
            del lst
        del a, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
