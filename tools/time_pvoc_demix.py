"""The stereo demix of Pvoc (pvoc_demix.hip: k_pvoc_demix, k_pvoc_demix_az) against the torch composition a caller writes
without it, which evaluates the same scan: the P + 1 gains broadcast against every bin, `min` with its index and `max`
along them, `where` for the side, the window and the frames, and `scatter_add_` for the azimuth profile (whose sums then
depend on the order the atomics land in).  The broadcast is P + 1 times the size of the amps, so the composition walks the
frames in chunks of about 1 GiB of it.  16 channels x 2^22 samples, hop = size / 4, P = 100, with and without the
profile.  Three medians per leg, the legs interleaved; algorithmic GB/s counts two streams in and one out (and the profile).
One JSON line per size, with the copy figure of the same box (bandwidth_probe) beside it.

    python tools/time_pvoc_demix.py [--sizes 256,2048,16384] [--channels 16] [--log2-samples 22] [--points 100] [--reps 10]
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
    ap.add_argument("--points", type=int, default=100)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sr", type=float, default=48000.0)
    args = ap.parse_args()
    C, samples, sr, P = args.channels, 1 << args.log2_samples, args.sr, args.points
    dev = "cuda:0"
    copy_tbs = fa.bandwidth_probe(0)["copy"]
    grid = torch.arange(P + 1, device=dev, dtype=torch.float32) / P
    for size in [int(s) for s in args.sizes.split(",")]:
        hop, M = size // 4, size // 2
        pv = fa.Pvoc(0, size, hop, sr, C)
        assert pv.get_error() == 0, pv.get_log()
        F = 1 + (samples - size) // hop
        g = torch.Generator(device=dev).manual_seed(size)
        # every bin a source at a random pan of a random side; freqs around the bin centres
        left = torch.rand((C, F, M + 1, 2), device=dev, generator=g) + 0.01
        right = torch.rand((C, F, M + 1, 2), device=dev, generator=g) + 0.01
        pan = torch.rand((C, F, M + 1), device=dev, generator=g)
        side = torch.rand((C, F, M + 1), device=dev, generator=g) < 0.5
        loud = left[..., 0].clone()
        left[..., 0] = torch.where(side, loud, loud * pan)
        right[..., 0] = torch.where(side, loud * pan, loud)
        for x in (left, right):
            x[..., 1] = (x[..., 1] - 0.51 + torch.arange(M + 1, device=dev)) * (sr / size)
        del pan, side, loud
        out = torch.empty_like(left)
        az = torch.empty((C, F, 2 * P + 1), device=dev)
        par = torch.empty((F, 2), device=dev)
        par[:, 0] = torch.linspace(-1, 1, F, device=dev)          # the window sweeps the stage
        par[:, 1] = 9.0
        c = torch.round(par[:, 0] * P).to(torch.int64)
        H = 4
        step = max(1, (1 << 28) // (C * (M + 1) * (P + 1)))         # frames per chunk: 2^28 floats of the broadcast
        out2, az2 = torch.empty_like(left), torch.empty_like(az)

        def compose(with_az):
            for f0 in range(0, F, step):
                f1 = min(F, f0 + step)
                L, R = left[:, f0:f1, :, 0], right[:, f0:f1, :, 0]
                isleft = L > R
                ld, qt = torch.where(isleft, L, R), torch.where(isleft, R, L)
                d = (qt[..., None] - grid * ld[..., None]).abs()
                m, nmin = d.min(-1)
                mag = d.max(-1).values - m
                u = torch.where(isleft, nmin - P, P - nmin)
                placed = mag > 0
                kept = placed & ((u - c[f0:f1, None]).abs() <= H)
                out2[:, f0:f1, :, 0] = torch.where(kept, mag, torch.zeros_like(mag))
                out2[:, f0:f1, :, 1] = torch.where(isleft, left[:, f0:f1, :, 1], right[:, f0:f1, :, 1])
                if with_az:
                    az2[:, f0:f1].zero_().scatter_add_(-1, u + P, torch.where(placed, mag, torch.zeros_like(mag)))

        legs = {"demix": lambda: pv.demix_device(left, right, out, par, P),
                "compose_demix": lambda: compose(False),
                "demix_az": lambda: pv.demix_device(left, right, out, par, P, az_out=az),
                "compose_demix_az": lambda: compose(True)}
        assert legs["demix"]() == 0 and legs["demix_az"]() == 0
        compose(True)
        torch.cuda.synchronize()
        # the two agree on which bins are kept, but for the bins whose smallest d is tied (torch's min may take either n)
        differ = int(((out[..., 0] != 0) != (out2[..., 0] != 0)).sum())
        assert differ <= out[..., 0].numel() // 1000, differ
        assert torch.allclose(az.sum(-1), az2.sum(-1), rtol=1e-4)
        t = interleaved(legs, args.reps)
        med = {k: float(np.median(v)) for k, v in t.items()}
        nbytes = 3 * left.numel() * 4
        azbytes = az.numel() * 4
        print(json.dumps({"size": size, "hop": hop, "channels": C, "frames": F, "points": P, "bytes": nbytes,
                          "az_bytes": azbytes, "kept_differ": differ,
                          "ms": {k: [round(u, 4) for u in v] for k, v in t.items()},
                          "gbs": {k: round((nbytes + (azbytes if k.endswith("az") else 0)) / med[k] / 1e6, 1) for k in legs},
                          "ratio": {"compose_over_demix": round(med["compose_demix"] / med["demix"], 2),
                                    "compose_over_demix_az": round(med["compose_demix_az"] / med["demix_az"], 2),
                                    "az_over_plain": round(med["demix_az"] / med["demix"], 2)},
                          "spread": {k: round((max(v) - min(v)) / med[k], 3) for k, v in t.items()},
                          "copy_gbs": round(copy_tbs * 1e3, 1),
                          "kernels": [pv.demix_kernel_name(), pv.demix_kernel_name(az=True)]}), flush=True)
        del left, right, out, az, out2, az2
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
