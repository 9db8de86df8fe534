"""The oscillator bank of Pvoc (pvoc_adsyn.hip, Pvoc.adsyn_device) against a torch composition a caller could write: over
blocks of frames, linear interpolation of amp and freq across the hop, float32 `cumsum` of the frequency into a phase
(carried from block to block), `cos`, and a sum over the bins.  The composition drifts and depends on its blocks; it is
timed, not compared.  16 channels x 2^20 samples, hop = size / 4, all bins and every 8th bin.  Three medians per leg, the
legs interleaved.  One JSON line per size and selection: oscillator-samples per second, and their share of the fp32
multiply-add peak (one multiply-add per oscillator-sample: CUs x 128 lanes x the clock the device reports, or --clock-mhz).

    python tools/time_pvoc_adsyn.py [--sizes 256,2048] [--channels 16] [--log2-samples 20] [--reps 3]
"""
import argparse
import json
import math
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
    ap.add_argument("--sizes", default="256,2048")
    ap.add_argument("--channels", type=int, default=16)
    ap.add_argument("--log2-samples", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sr", type=float, default=48000.0)
    ap.add_argument("--clock-mhz", type=float, default=2400.0, help="used where the device reports no clock (MI355X: 2400)")
    ap.add_argument("--block-elements", type=int, default=1 << 26, help="elements of one temporary of the composition")
    args = ap.parse_args()
    C, samples, sr = args.channels, 1 << args.log2_samples, args.sr
    dev = "cuda:0"
    prop = torch.cuda.get_device_properties(0)
    clock_hz = float(getattr(prop, "clock_rate", 0)) * 1e3 or args.clock_mhz * 1e6
    peak = prop.multi_processor_count * 128 * clock_hz      # fp32 multiply-adds per second
    for size in [int(s) for s in args.sizes.split(",")]:
        hop, M = size // 4, size // 2
        F = samples // hop
        pv = fa.Pvoc(0, size, hop, sr, C)
        assert pv.get_error() == 0, pv.get_log()
        g = torch.Generator(device=dev).manual_seed(size)
        frames = torch.rand((C, F, M + 1, 2), device=dev, generator=g)
        frames[..., 1] = (torch.arange(M + 1, device=dev) + frames[..., 1] - 0.5) * (sr / size) * 0.999
        out = torch.empty((C, F * hop), device=dev)
        ref = torch.empty((C, F * hop), device=dev)
        w = (torch.arange(1, hop + 1, device=dev, dtype=torch.float32) / hop)[None, None, :, None]
        for step in (1, 8):
            bins = torch.arange(0, M + 1, step, device=dev)
            nb = bins.numel()
            fb = max(1, min(F, args.block_elements // (C * hop * nb)))

            def compose():
                a_prev = torch.zeros((C, 1, nb), device=dev)
                f_prev = frames[:, :1, bins, 1]
                phase = torch.zeros((C, 1, nb), device=dev)
                for f0 in range(0, F, fb):
                    blk = frames[:, f0:f0 + fb][:, :, bins]
                    a1, f1 = blk[..., 0], blk[..., 1]
                    a0, fq0 = torch.cat([a_prev, a1[:, :-1]], dim=1), torch.cat([f_prev, f1[:, :-1]], dim=1)
                    n = a1.shape[1]
                    amp = (a0[:, :, None] + (a1 - a0)[:, :, None] * w).reshape(C, n * hop, nb)
                    inc = ((fq0[:, :, None] + (f1 - fq0)[:, :, None] * w) * (2 * math.pi / sr)).reshape(C, n * hop, nb)
                    ph = torch.cumsum(inc, dim=1) + phase
                    ref[:, f0 * hop:(f0 + n) * hop] = (amp * torch.cos(ph)).sum(dim=-1)
                    a_prev, f_prev, phase = a1[:, -1:], f1[:, -1:], torch.remainder(ph[:, -1:], 2 * math.pi)
                return ref

            legs = {"adsyn": lambda: pv.adsyn_device(frames, out, first_bin=0, nbins=nb, step=step), "compose": compose}
            assert legs["adsyn"]() == 0
            t = interleaved(legs, args.reps)
            med = {n: float(np.median(v)) for n, v in t.items()}
            work = float(C) * F * hop * nb
            print(json.dumps({"size": size, "hop": hop, "channels": C, "frames": F, "step": step, "oscillators": nb,
                              "oscillator_samples": work, "compose_block_frames": fb,
                              "ms": {n: [round(u, 3) for u in v] for n, v in t.items()},
                              "gosc_per_s": {n: round(work / med[n] / 1e6, 2) for n in legs},
                              "fma_peak_share": {n: round(work / (med[n] * 1e-3) / peak, 4) if peak else None for n in legs},
                              "ratio_compose_over_adsyn": round(med["compose"] / med["adsyn"], 2),
                              "spread": {n: round((max(v) - min(v)) / med[n], 3) for n, v in t.items()},
                              "clock_mhz": clock_hz / 1e6, "cus": prop.multi_processor_count,
                              "kernel": pv.adsyn_kernel_name()}), flush=True)
        del frames, out, ref
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
