"""The phase vocoder's conversions (Pvoc, pvoc_kernels.hip) against the torch composition a caller writes today: analysis =
layout map, abs, angle of the product with the previous frame and the expected advance, scale; synthesis = wrap, a float32
cumsum of phases over the frames, polar, layout map back.  16 channels x 2^22 samples, hop = size / 4.  Three medians per
leg, the legs interleaved; algorithmic GB/s counts the spectra and the frames once each.  One JSON line per size.

    python tools/time_pvoc.py [--sizes 256,2048,16384] [--channels 16] [--log2-samples 22] [--reps 10]
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


def median_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def interleaved(legs, reps, rounds=3):
    """{name: [median of `reps` runs, one per round]}, the legs taking turns within every round"""
    for fn in legs.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            out[k].append(median_ms(fn, reps))
    return out


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
    x = torch.rand((C, samples), device=dev) * 2 - 1
    for size in [int(s) for s in args.sizes.split(",")]:
        hop, M = size // 4, size // 2
        w = torch.from_numpy((0.5 - 0.5 * np.cos(2 * np.pi * np.arange(size) / size)).astype(np.float32)).to(dev)
        an = fa.Stft(0, size, hop, window=w)
        pv = fa.Pvoc(0, size, hop, sr, C)
        assert an.get_error() == 0 and pv.get_error() == 0, pv.get_log()
        F = an.frames(samples)
        spec = torch.empty((C, F, M), dtype=torch.complex64, device=dev)
        assert an.analyze_device(x, spec) == 0
        frames = torch.empty((C, F, M + 1, 2), device=dev)
        back = torch.empty_like(spec)
        assert pv.analyze_device(spec, frames) == 0 and pv.synthesize_device(frames, back) == 0   # (allocates the workspace)
        torch.cuda.synchronize()

        k = torch.arange(M + 1, device=dev)
        e = torch.polar(torch.ones(M + 1, device=dev), (-2 * math.pi / size) * ((k * hop) % size).float())
        kf32, sh, srs, kf = k.float(), float(size / hop), float(sr / size), float(hop / sr)
        prev = torch.ones((C, 1, M + 1), dtype=torch.complex64, device=dev)
        ph0 = torch.zeros((C, 1, M + 1), device=dev)

        def comp_analyze():
            z = torch.cat([spec, spec[..., :1].imag.to(torch.complex64)], dim=-1)
            z[..., 0] = spec[..., 0].real
            z[..., M // 2] = spec[..., M // 2].conj()
            d = z * torch.cat([prev, z[:, :-1]], dim=1).conj() * e
            return torch.stack([z.abs(), (kf32 + d.angle() * (sh / (2 * math.pi))) * srs], dim=-1)

        def comp_synth():
            t = frames[..., 1] * kf
            ph = torch.cumsum(t - torch.round(t), dim=1) + ph0
            z = torch.polar(frames[..., 0], ph * (2 * math.pi))
            P = z[..., :M].clone()
            P[..., 0] = torch.complex(z[..., 0].real, z[..., M].real)
            P[..., M // 2] = z[..., M // 2].conj()
            return P

        legs = {"analyze": lambda: pv.analyze_device(spec, frames), "compose_analyze": comp_analyze,
                "synth": lambda: pv.synthesize_device(frames, back), "compose_synth": comp_synth}
        t = interleaved(legs, args.reps)
        med = {k: float(np.median(v)) for k, v in t.items()}
        spread = {k: (max(v) - min(v)) / med[k] for k, v in t.items()}
        nbytes = spec.numel() * 8 + frames.numel() * 4
        print(json.dumps({"size": size, "hop": hop, "channels": C, "frames": F, "bytes": nbytes,
                          "ms": {k: [round(u, 4) for u in v] for k, v in t.items()},
                          "analyze_gbs": round(nbytes / med["analyze"] / 1e6, 1),
                          "synth_gbs": round(nbytes / med["synth"] / 1e6, 1),
                          "compose_analyze_gbs": round(nbytes / med["compose_analyze"] / 1e6, 1),
                          "compose_synth_gbs": round(nbytes / med["compose_synth"] / 1e6, 1),
                          "analyze_speedup": round(med["compose_analyze"] / med["analyze"], 2),
                          "synth_speedup": round(med["compose_synth"] / med["synth"], 2),
                          "spread": {k: round(v, 3) for k, v in spread.items()},
                          "workspace_bytes": pv.workspace_bytes()}), flush=True)
        del spec, frames, back
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
