"""The two-input frame operations of Pvoc (pvoc_pair.hip: cross, morph, filter, mix, vocode) against the torch composition
a caller writes without them: elementwise tensor expressions for the first four, torch.fft (rfft of the even extension of
the log amps, lifter, irfft) for the vocoder's two envelopes.  16 channels x 2^22 samples, hop = size / 4.  Three medians
per leg, the legs interleaved; algorithmic GB/s counts the two input streams and the output once each.  One JSON line per
size, with the copy figure of the same box (bandwidth_probe) beside it.

    python tools/time_pvoc_pair.py [--sizes 256,2048,16384] [--channels 16] [--log2-samples 22] [--reps 10] [--coefs 80]
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
    ap.add_argument("--coefs", type=int, default=80)
    ap.add_argument("--sr", type=float, default=48000.0)
    args = ap.parse_args()
    C, samples, sr = args.channels, 1 << args.log2_samples, args.sr
    dev = "cuda:0"
    copy_tbs = fa.bandwidth_probe(0)["copy"]
    for size in [int(s) for s in args.sizes.split(",")]:
        hop, M = size // 4, size // 2
        coefs = min(args.coefs, M - 1)
        pv = fa.Pvoc(0, size, hop, sr, C)
        assert pv.get_error() == 0, pv.get_log()
        F = 1 + (samples - size) // hop
        g = torch.Generator(device=dev).manual_seed(size)
        a = torch.rand((C, F, M + 1, 2), device=dev, generator=g) + 0.01
        b = torch.rand((C, F, M + 1, 2), device=dev, generator=g) + 0.01
        out = torch.empty_like(a)
        p = torch.full((F,), 0.6, device=dev)
        q = torch.full((F,), 0.9, device=dev)
        P, Q = p[None, :, None], q[None, :, None]

        def envelope(amp):
            L = torch.log(torch.clamp(amp, min=1e-20))
            X = torch.fft.rfft(torch.cat([L, L[..., 1:M].flip(-1)], dim=-1), dim=-1)
            X[..., coefs + 1:] = 0
            return torch.exp(torch.fft.irfft(X.real.to(torch.complex64), n=size, dim=-1)[..., :M + 1])

        def comp_cross():
            return torch.stack([a[..., 0] * P + b[..., 0] * Q, a[..., 1]], dim=-1)

        def comp_morph():
            return torch.stack([torch.lerp(a[..., 0], b[..., 0], P), torch.lerp(a[..., 1], b[..., 1], Q)], dim=-1)

        def comp_filter():
            return torch.stack([Q * (a[..., 0] * ((1 - P) + P * b[..., 0])), a[..., 1]], dim=-1)

        def comp_mix():
            return torch.where((b[..., 0] > a[..., 0])[..., None], b, a)

        def comp_vocode():
            r = envelope(a[..., 0]) / envelope(b[..., 0])
            return torch.stack([Q * (b[..., 0] * ((1 - P) + P * r)), b[..., 1]], dim=-1)

        legs = {"cross": lambda: pv.cross_device(a, b, out, p, q), "compose_cross": comp_cross,
                "morph": lambda: pv.morph_device(a, b, out, p, q), "compose_morph": comp_morph,
                "filter": lambda: pv.filter_device(a, b, out, p, q), "compose_filter": comp_filter,
                "mix": lambda: pv.mix_device(a, b, out), "compose_mix": comp_mix,
                "vocode": lambda: pv.vocode_device(a, b, out, p, q, coefs=coefs), "compose_vocode": comp_vocode}
        t = interleaved(legs, args.reps)
        med = {n: float(np.median(v)) for n, v in t.items()}
        nbytes = 3 * a.numel() * 4
        ours = [n for n in legs if not n.startswith("compose_")]
        print(json.dumps({"size": size, "hop": hop, "channels": C, "frames": F, "coefs": coefs, "bytes": nbytes,
                          "ms": {n: [round(u, 4) for u in v] for n, v in t.items()},
                          "gbs": {n: round(nbytes / med[n] / 1e6, 1) for n in legs},
                          "speedup": {n: round(med["compose_" + n] / med[n], 2) for n in ours},
                          "spread": {n: round((max(v) - min(v)) / med[n], 3) for n, v in t.items()},
                          "copy_gbs": round(copy_tbs * 1e3, 1),
                          "kernels": [pv.pair_kernel_name("cross"), pv.pair_kernel_name("vocode")]}), flush=True)
        del a, b, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
