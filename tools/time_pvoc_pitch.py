"""The pitch of Pvoc (pitch_kernels.hip: k_pvoc_pitch) against the torch composition of the same definition that a caller
writes without it: shifted comparisons for the peak mask, cumsum + scatter for the list, the candidates x peaks broadcast
in chunks of frames, max.  (The composition sums a candidate's terms with torch.sum and breaks ties as max does: it is
what a caller would write, not the definition's bits; the share of the frames in which the two agree on F0 within 3 % is reported.)
16 channels x 2^22 samples, hop = size / 4, npeaks = 16, with and without the peak list, on two kinds of frames: `tones`
(12 partials over a low floor, thresh above the floor: the walk reads the whole frame) and `noise` (random amps, thresh
0: a peak every few bins, the walk stops after the first rows).  Three medians per leg, the legs interleaved; algorithmic
GB/s counts the frames in.  One JSON line per size and kind, with the read figure of the same box (bandwidth_probe)
beside it: the kernel reads a stream and writes next to nothing.

    python tools/time_pvoc_pitch.py [--sizes 256,2048,16384] [--channels 16] [--log2-samples 22] [--reps 10]
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

NPEAKS, TOL, DECAY = 16, 0.03, 0.84


def compose(a, rows, thresh, fmin, fmax, w, chunk_elems=1 << 26):
    """the torch composition: rows (C, F, 4) <- frames a (C, F, M + 1, 2)"""
    amp, q = a[..., 0], a[..., 1]
    mid, qm = amp[..., 1:-1], q[..., 1:-1]
    pk = (mid > amp[..., :-2]) & (mid >= amp[..., 2:]) & (mid >= thresh) & torch.isfinite(qm) & (qm > 0)
    place = pk.cumsum(-1) - 1
    idx = torch.where(pk & (place < NPEAKS), place, NPEAKS)          # the slot past the list takes what is not in it
    A = torch.zeros(a.shape[:2] + (NPEAKS + 1,), device=a.device).scatter_(-1, idx, mid)[..., :NPEAKS]
    Q = torch.zeros(a.shape[:2] + (NPEAKS + 1,), device=a.device).scatter_(-1, idx, qm)[..., :NPEAKS]
    L = pk.sum(-1).clamp(max=NPEAKS)
    have = torch.arange(NPEAKS, device=a.device) < L[..., None]
    div = torch.arange(1, 9, device=a.device, dtype=torch.float32)
    C, F = a.shape[:2]
    step = max(1, chunk_elems // (C * NPEAKS * 8 * NPEAKS))
    for f0 in range(0, F, step):
        Af, Qf, hf = A[:, f0:f0 + step], Q[:, f0:f0 + step], have[:, f0:f0 + step]
        cand = (Qf[..., None] / div).flatten(-2)                                  # (C, f, 8 NPEAKS)
        valid = hf[..., None].expand(-1, -1, -1, 8).flatten(-2) & (cand >= fmin) & (cand <= fmax)
        r = Qf[..., None, :] / cand[..., None]                                    # (C, f, 8 NPEAKS, NPEAKS)
        h = r.round()
        ok = (h >= 1) & (h <= 32) & ((r - h).abs() / h <= TOL) & hf[..., None, :]
        s = torch.where(ok, Af[..., None, :] * w[torch.where(ok, h - 1, 0.0).long()], 0.0).sum(-1)
        s = torch.where(valid & ~s.isnan(), s, -1.0)
        smax, arg = s.max(-1)
        found = smax >= 0
        total = Af.sum(-1)
        out = rows[:, f0:f0 + step]
        out[..., 0] = torch.where(found, cand.gather(-1, arg[..., None])[..., 0], 0.0)
        out[..., 1] = torch.where(found, smax, 0.0)
        out[..., 2] = torch.where(found & (total != 0), smax / total, 0.0)
        out[..., 3] = L[:, f0:f0 + step]
    return rows


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
    w = torch.tensor([float(np.float32(DECAY)) ** h for h in range(32)], dtype=torch.float32, device=dev)
    for size in [int(s) for s in args.sizes.split(",")]:
        hop, M = size // 4, size // 2
        pv = fa.Pvoc(0, size, hop, sr, C)
        assert pv.get_error() == 0, pv.get_log()
        F = 1 + (samples - size) // hop
        g = torch.Generator(device=dev).manual_seed(size)
        fmin, fmax = 2 * sr / size, sr / 4
        for kind in ("tones", "noise"):
            a = torch.rand((C, F, M + 1, 2), device=dev, generator=g) + 0.01
            a[..., 1] = (a[..., 1] - 0.51 + torch.arange(M + 1, device=dev)) * (sr / size)      # freqs around the bin centres
            thresh = 0.0
            if kind == "tones":       # 12 partials of a fundamental near bin M / 16, which moves with the frame
                a[..., 0] *= 1e-3
                k0 = M / 16 * (1 + 0.2 * torch.rand((C, F), device=dev, generator=g))
                for h in range(1, 13):
                    k = (k0 * h).round().long().clamp(max=M - 1)[..., None]
                    a[..., 0].scatter_(-1, k, 1.0 / h)
                    a[..., 1].scatter_(-1, k, (k0 * h * (sr / size))[..., None])
                thresh = 0.01
            rows, ref = torch.empty((C, F, 4), device=dev), torch.empty((C, F, 4), device=dev)
            lst = torch.empty((C, F, NPEAKS, 2), device=dev)
            legs = {"pitch": lambda: pv.pitch_device(a, rows, thresh, fmin, fmax, NPEAKS, TOL, DECAY),
                    "compose_pitch": lambda: compose(a, ref, thresh, fmin, fmax, w),
                    "pitch_list": lambda: pv.pitch_device(a, rows, thresh, fmin, fmax, NPEAKS, TOL, DECAY, peaks_out=lst)}
            assert legs["pitch"]() == 0 and legs["pitch_list"]() == 0
            legs["compose_pitch"]()
            torch.cuda.synchronize()
            agree = float(((rows[..., 0] - ref[..., 0]).abs() <= 0.03 * ref[..., 0]).float().mean())
            t = interleaved(legs, args.reps)
            med = {k: float(np.median(v)) for k, v in t.items()}
            nbytes = a.numel() * 4
            print(json.dumps({"size": size, "hop": hop, "channels": C, "frames": F, "kind": kind, "npeaks": NPEAKS,
                              "bytes": nbytes, "mean_peaks": round(float(rows[..., 3].mean()), 2), "f0_agree": round(agree, 4),
                              "ms": {k: [round(u, 4) for u in v] for k, v in t.items()},
                              "gbs": {k: round(nbytes / med[k] / 1e6, 1) for k in legs},
                              "ratio": {"compose_over_pitch": round(med["compose_pitch"] / med["pitch"], 2)},
                              "spread": {k: round((max(v) - min(v)) / med[k], 3) for k, v in t.items()},
                              "read_gbs": round(read_tbs * 1e3, 1),
                              "kernels": [pv.pitch_kernel_name()]}), flush=True)
            del a, rows, ref, lst
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
