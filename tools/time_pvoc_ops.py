"""The frame operations of Pvoc (pvoc_ops.hip: pitch scale, frequency shift, timed read) against the torch composition a
caller writes today: round / scatter for the source map, torch.fft (rfft of the even extension of the log amps, lifter,
irfft) for the formant envelope, lerp of gathered frames for the read.  16 channels x 2^22 samples, hop = size / 4.  Three
medians per leg, the legs interleaved; algorithmic GB/s counts the frames in and the frames out once each.  One JSON line
per size.  Nothing here has been measured yet: the tool exists so that it can be.

    python tools/time_pvoc_ops.py [--sizes 256,2048,16384] [--channels 16] [--log2-samples 22] [--reps 10] [--coefs 80]
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
    for size in [int(s) for s in args.sizes.split(",")]:
        hop, M = size // 4, size // 2
        coefs = min(args.coefs, M - 1)
        pv = fa.Pvoc(0, size, hop, sr, C)
        assert pv.get_error() == 0, pv.get_log()
        F = 1 + (samples - size) // hop
        g = torch.Generator(device=dev).manual_seed(size)
        frames = torch.rand((C, F, M + 1, 2), device=dev, generator=g) + 0.01
        out = torch.empty_like(frames)
        s = torch.full((F,), 1.31, device=dev)
        hz = torch.full((F,), 5.0 * sr / size, device=dev)
        pos = torch.arange(F, device=dev, dtype=torch.float32) * 0.75
        cf = float(np.float32(sr / size))
        centre = torch.arange(M + 1, device=dev, dtype=torch.float32) * cf
        k = torch.arange(1, M, device=dev)

        def envelope(amp):
            L = torch.log(torch.clamp(amp, min=1e-20))
            X = torch.fft.rfft(torch.cat([L, L[..., 1:M].flip(-1)], dim=-1), dim=-1)
            X[..., coefs + 1:] = 0
            return torch.exp(torch.fft.irfft(X.real.to(torch.complex64), n=size, dim=-1)[..., :M + 1])

        def comp_scale(keepform):
            amp, freq = frames[..., 0], frames[..., 1]
            a = amp / envelope(amp) if keepform else amp
            j = torch.floor(k.float() * 1.31 + 0.5).long()
            ok = (j >= 1) & (j <= M - 1)
            oa = torch.zeros_like(amp)
            of = centre.expand_as(freq).clone()
            # (equal indices: the composition does not even fix which source wins)
            oa[..., j[ok]] = a[..., k[ok]]
            of[..., j[ok]] = freq[..., k[ok]] * 1.31
            if keepform:
                oa = oa * envelope(amp)
            oa[..., 0], oa[..., M], of[..., 0], of[..., M] = amp[..., 0], amp[..., M], freq[..., 0], freq[..., M]
            return torch.stack([oa, of], dim=-1)

        def comp_shift(keepform):
            amp, freq = frames[..., 0], frames[..., 1]
            a = amp / envelope(amp) if keepform else amp
            oa = torch.zeros_like(amp)
            of = centre.expand_as(freq).clone()
            oa[..., 6:M] = a[..., 1:M - 5]
            of[..., 6:M] = freq[..., 1:M - 5] + 5.0 * sr / size
            if keepform:
                oa = oa * envelope(amp)
            oa[..., 0], oa[..., M], of[..., 0], of[..., M] = amp[..., 0], amp[..., M], freq[..., 0], freq[..., M]
            return torch.stack([oa, of], dim=-1)

        def comp_read():
            p = pos.clamp(0, F - 1)
            i = p.floor().long()
            i1 = (i + 1).clamp(max=F - 1)
            return torch.lerp(frames[:, i], frames[:, i1], (p - i.float())[None, :, None, None])

        legs = {"scale": lambda: pv.scale_device(frames, out, s), "compose_scale": lambda: comp_scale(False),
                "scale_keepform": lambda: pv.scale_device(frames, out, s, keepform=True, coefs=coefs),
                "compose_scale_keepform": lambda: comp_scale(True),
                "shift": lambda: pv.shift_device(frames, out, hz), "compose_shift": lambda: comp_shift(False),
                "shift_keepform": lambda: pv.shift_device(frames, out, hz, keepform=True, coefs=coefs),
                "compose_shift_keepform": lambda: comp_shift(True),
                "read": lambda: pv.read_device(frames, pos, out), "compose_read": comp_read}
        t = interleaved(legs, args.reps)
        med = {n: float(np.median(v)) for n, v in t.items()}
        nbytes = 2 * frames.numel() * 4
        ours = [n for n in legs if not n.startswith("compose_")]
        print(json.dumps({"size": size, "hop": hop, "channels": C, "frames": F, "coefs": coefs, "bytes": nbytes,
                          "ms": {n: [round(u, 4) for u in v] for n, v in t.items()},
                          "gbs": {n: round(nbytes / med[n] / 1e6, 1) for n in legs},
                          "speedup": {n: round(med["compose_" + n] / med[n], 2) for n in ours},
                          "spread": {n: round((max(v) - min(v)) / med[n], 3) for n, v in t.items()},
                          "kernels": [pv.ops_kernel_name("scale"), pv.ops_kernel_name("scale", True),
                                      pv.ops_kernel_name("read")]}), flush=True)
        del frames, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
