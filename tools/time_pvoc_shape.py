"""The one-stream shaping operations of Pvoc (pvoc_shape.hip: band, mask, stencil, arp, lock, warp) against the torch
composition a caller writes without them: where / clamp arithmetic for the band, one or two elementwise expressions for
mask, stencil and arp, a max_pool1d peak mask plus shifted where for the lock, torch.fft (rfft of the even extension of
the log amps, lifter, irfft) plus a gather for the warp (its index map built once, outside the timed leg).  16 channels x
2^22 samples, hop = size / 4.  Three medians per leg, the legs interleaved; algorithmic GB/s counts the input stream and
the output once each.  One JSON line per size, with the copy figure of the same box (bandwidth_probe) beside it.

    python tools/time_pvoc_shape.py [--sizes 256,2048,16384] [--channels 16] [--log2-samples 22] [--reps 10] [--coefs 80]
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
        a[..., 1] = (a[..., 1] - 0.51 + torch.arange(M + 1, device=dev)) * (sr / size)      # freqs around the bin centres
        out = torch.empty_like(a)
        table = torch.rand((M + 1,), device=dev, generator=g)
        full = lambda v: torch.full((F,), v, device=dev)
        lc, lf, hf, hc = full(500.0), full(2000.0), full(8000.0), full(12000.0)
        depth, gain, level, pos, tol, lock = full(0.6), full(0.9), full(0.5), full(0.37), full(0.01), full(1.0)
        scale, shift = full(1.37), full(3.4 * sr / size)
        col = lambda v: v[None, :, None]
        bins = torch.arange(M + 1, device=dev)
        # the warp's map, once: bin j looks at the scale map's source of bin j - d (nearest k with round(k s) == j - d)
        jj = bins - int(round(3.4))
        k = torch.clamp(torch.round(jj / 1.37), 1, M - 1).long()
        hit = (torch.floor(k * 1.37 + 0.5).long() == jj) & (jj >= 1) & (jj <= M - 1) & (bins >= 1) & (bins <= M - 1)
        src = torch.where(hit, k, bins)[None, None, :].expand(C, F, M + 1)

        def envelope(amp):
            L = torch.log(torch.clamp(amp, min=1e-20))
            X = torch.fft.rfft(torch.cat([L, L[..., 1:M].flip(-1)], dim=-1), dim=-1)
            X[..., coefs + 1:] = 0
            return torch.exp(torch.fft.irfft(X.real.to(torch.complex64), n=size, dim=-1)[..., :M + 1])

        def comp_band():
            x = a[..., 1].abs()
            up, down = (x - col(lc)) / (col(lf) - col(lc)), (col(hc) - x) / (col(hc) - col(hf))
            return torch.stack([a[..., 0] * torch.clamp(torch.minimum(up, down), 0, 1), a[..., 1]], dim=-1)

        def comp_mask():
            return torch.stack([a[..., 0] * ((1 - col(depth)) + col(depth) * table), a[..., 1]], dim=-1)

        def comp_stencil():
            amp = a[..., 0]
            return torch.stack([torch.where(amp < table * col(level), amp * col(gain), amp), a[..., 1]], dim=-1)

        def comp_arp():
            t = torch.floor(pos * M).long()
            m = torch.where(bins[None, :] == t[:, None], gain[:, None], 1 - depth[:, None])
            return torch.stack([a[..., 0] * m[None], a[..., 1]], dim=-1)

        def comp_lock():
            amp, freq = a[..., 0], a[..., 1]
            pk = amp == torch.nn.functional.max_pool1d(amp, 5, 1, 2)
            up, down = torch.roll(pk, -1, -1), torch.roll(pk, 1, -1)
            Fc = torch.where(up, torch.roll(freq, -1, -1), torch.roll(freq, 1, -1))
            take = (up | down) & ((freq - Fc).abs() < col(tol) * Fc.abs()) & (col(lock) != 0)
            return torch.stack([amp, torch.where(take, Fc, freq)], dim=-1)

        def comp_warp():
            amp = a[..., 0]
            env = envelope(amp)
            moved = col(gain) * amp / env * torch.gather(env, -1, src)
            return torch.stack([torch.where(hit, moved, col(gain) * amp), a[..., 1]], dim=-1)

        legs = {"band": lambda: pv.band_device(a, out, lc, lf, hf, hc), "compose_band": comp_band,
                "mask": lambda: pv.mask_device(a, out, table, depth), "compose_mask": comp_mask,
                "stencil": lambda: pv.stencil_device(a, out, table, gain, level), "compose_stencil": comp_stencil,
                "arp": lambda: pv.arp_device(a, out, pos, depth, gain), "compose_arp": comp_arp,
                "lock": lambda: pv.lock_device(a, out, lock, tol), "compose_lock": comp_lock,
                "warp": lambda: pv.warp_device(a, out, scale, shift, 1, gain, coefs), "compose_warp": comp_warp}
        for name in ("band", "mask", "stencil", "arp", "lock", "warp"):
            assert legs[name]() == 0, name
        t = interleaved(legs, args.reps)
        med = {n: float(np.median(v)) for n, v in t.items()}
        nbytes = 2 * a.numel() * 4
        ours = [n for n in legs if not n.startswith("compose_")]
        print(json.dumps({"size": size, "hop": hop, "channels": C, "frames": F, "coefs": coefs, "bytes": nbytes,
                          "ms": {n: [round(u, 4) for u in v] for n, v in t.items()},
                          "gbs": {n: round(nbytes / med[n] / 1e6, 1) for n in legs},
                          "speedup": {n: round(med["compose_" + n] / med[n], 2) for n in ours},
                          "spread": {n: round((max(v) - min(v)) / med[n], 3) for n, v in t.items()},
                          "copy_gbs": round(copy_tbs * 1e3, 1),
                          "kernels": [pv.shape_kernel_name(n) for n in ("band", "lock", "warp")]}), flush=True)
        del a, out, src
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
