"""The per-frame descriptors of Pvoc (pvoc_desc.hip: k_pvoc_desc) against the plain torch composition a caller writes
without them: three sums over the bins (amp, amp^2, amp x bin centre), a division, a shifted difference with its sum, max
and a gather of the peak's freq.  16 channels x 2^22 samples, hop = size / 4.  Three medians per leg, the legs
interleaved; algorithmic GB/s counts the input stream once (the rows written are 32 bytes per frame).  A third leg runs
the descriptors over half the bins (a ranged call loads only its range).  One JSON line per size, with the read figure of
the same box (bandwidth_probe) beside it: the kernel reads, it hardly writes.

    python tools/time_pvoc_desc.py [--sizes 256,2048,16384] [--channels 16] [--log2-samples 22] [--reps 10]
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
    read_tbs = fa.bandwidth_probe(0)["read"]
    for size in [int(s) for s in args.sizes.split(",")]:
        hop, M = size // 4, size // 2
        pv = fa.Pvoc(0, size, hop, sr, C)
        assert pv.get_error() == 0, pv.get_log()
        F = 1 + (samples - size) // hop
        g = torch.Generator(device=dev).manual_seed(size)
        a = torch.rand((C, F, M + 1, 2), device=dev, generator=g) + 0.01
        a[..., 1] = (a[..., 1] - 0.51 + torch.arange(M + 1, device=dev)) * (sr / size)      # freqs around the bin centres
        out = torch.empty((C, F, 8), device=dev)
        w = torch.arange(M + 1, device=dev, dtype=torch.float32) * (sr / size)
        last = torch.zeros((C, 1, M + 1), device=dev)

        def compose():
            amp = a[..., 0]
            mag, pw, mom = amp.sum(-1), (amp * amp).sum(-1), (amp * w).sum(-1)
            d = amp - torch.cat([last, amp[:, :-1]], dim=1)
            top, kp = amp.max(-1)
            freq = torch.gather(a[..., 1], -1, kp[..., None])[..., 0]
            return torch.stack([mag, pw, mom, mom / mag, (d * d).sum(-1), top, freq, kp.float()], dim=-1)

        legs = {"describe": lambda: pv.describe_device(a, out), "compose_describe": compose,
                "describe_half": lambda: pv.describe_device(a, out, M // 4, M // 2)}
        assert legs["describe"]() == 0 and legs["describe_half"]() == 0
        t = interleaved(legs, args.reps)
        med = {n: float(np.median(v)) for n, v in t.items()}
        nbytes = a.numel() * 4
        print(json.dumps({"size": size, "hop": hop, "channels": C, "frames": F, "bytes": nbytes,
                          "ms": {n: [round(u, 4) for u in v] for n, v in t.items()},
                          "gbs": {n: round(nbytes / med[n] / 1e6, 1) for n in ("describe", "compose_describe")},
                          "speedup": {"describe": round(med["compose_describe"] / med["describe"], 2)},
                          "half_over_all": round(med["describe_half"] / med["describe"], 3),
                          "spread": {n: round((max(v) - min(v)) / med[n], 3) for n, v in t.items()},
                          "read_gbs": round(read_tbs * 1e3, 1),
                          "kernels": [pv.desc_kernel_name()]}), flush=True)
        del a, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
