"""The operations along the frames of Pvoc (pvoc_time.hip: blur, smooth, freeze) against the torch composition a caller
writes without them.  16 channels x 2^22 samples, hop = size / 4.  Three medians per leg, the legs interleaved; algorithmic
GB/s counts the input stream and the output once each.  One JSON line per size, with the copy figure of the same box
(bandwidth_probe) beside it.

  blur    at n = 4 and n = 64 (max_frames 64) against torch.nn.functional.avg_pool1d over the frame axis (the frames moved
          to the last axis and back, which is what avg_pool1d asks for; the stream's start padded with zeros).
  freeze  a random half of the frames frozen, per column, against torch.cummax of the unfrozen frame indices plus a gather.
  smooth  the recurrence has no torch primitive: a Python loop of torch.lerp over the frames, timed on a shorter stream
          (--loop-frames) beside the kernel on the same shorter stream; `us_per_frame` says what a frame costs each side.
          The kernel is also timed on the whole stream.

    python tools/time_pvoc_time.py [--sizes 256,2048,16384] [--channels 16] [--log2-samples 22] [--reps 10] [--loop-frames 256]
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
    ap.add_argument("--loop-frames", type=int, default=256)
    ap.add_argument("--sr", type=float, default=48000.0)
    args = ap.parse_args()
    C, samples, sr = args.channels, 1 << args.log2_samples, args.sr
    dev = "cuda:0"
    copy_tbs = fa.bandwidth_probe(0)["copy"]
    for size in [int(s) for s in args.sizes.split(",")]:
        hop, M = size // 4, size // 2
        pv = fa.Pvoc(0, size, hop, sr, C)
        assert pv.get_error() == 0, pv.get_log()
        assert pv.blur_setup(64) == 0
        F = 1 + (samples - size) // hop
        Fs = min(args.loop_frames, F)
        g = torch.Generator(device=dev).manual_seed(size)
        a = torch.rand((C, F, M + 1, 2), device=dev, generator=g) + 0.01
        out = torch.empty_like(a)
        short, short_out = a[:, :Fs].contiguous(), torch.empty((C, Fs, M + 1, 2), device=dev)
        n4, n64 = torch.full((F,), 4.0, device=dev), torch.full((F,), 64.0, device=dev)
        wa, wf = torch.full((F,), 0.1, device=dev), torch.full((F,), 0.3, device=dev)
        wa_s, wf_s = wa[:Fs].contiguous(), wf[:Fs].contiguous()
        za = (torch.rand((F,), device=dev, generator=g) < 0.5).float()
        zf = (torch.rand((F,), device=dev, generator=g) < 0.5).float()
        frame_index = torch.arange(F, device=dev)

        def comp_blur(n):
            rows = a.permute(0, 2, 3, 1).reshape(-1, 1, F)
            avg = torch.nn.functional.avg_pool1d(torch.nn.functional.pad(rows, (n - 1, 0)), n, 1)
            return avg.reshape(C, M + 1, 2, F).permute(0, 3, 1, 2).contiguous()

        def comp_freeze():
            ga = torch.cummax(torch.where(za == 0, frame_index, 0), 0).values
            gf = torch.cummax(torch.where(zf == 0, frame_index, 0), 0).values
            return torch.stack([a[:, ga, :, 0], a[:, gf, :, 1]], dim=-1)

        def comp_smooth_loop():
            y, rows = torch.zeros((C, M + 1, 2), device=dev), []
            w = torch.stack([wa_s, wf_s], dim=-1)
            for f in range(Fs):
                y = torch.lerp(y, short[:, f], w[f])
                rows.append(y)
            return torch.stack(rows, dim=1)

        legs = {"blur4": lambda: pv.blur_device(a, out, n4), "compose_blur4": lambda: comp_blur(4),
                "blur64": lambda: pv.blur_device(a, out, n64), "compose_blur64": lambda: comp_blur(64),
                "freeze": lambda: pv.freeze_device(a, out, za, zf), "compose_freeze": comp_freeze,
                "smooth_short": lambda: pv.smooth_device(short, short_out, wa_s, wf_s), "compose_smooth_short": comp_smooth_loop,
                "smooth": lambda: pv.smooth_device(a, out, wa, wf)}
        t = interleaved(legs, args.reps)
        med = {n: float(np.median(v)) for n, v in t.items()}
        nbytes = 2 * a.numel() * 4
        sbytes = 2 * short.numel() * 4
        size_of = {n: sbytes if n.endswith("_short") else nbytes for n in legs}
        ours = [n for n in legs if not n.startswith("compose_") and "compose_" + n in legs]
        print(json.dumps({"size": size, "hop": hop, "channels": C, "frames": F, "loop_frames": Fs, "bytes": nbytes,
                          "lanes_smooth": C * (M + 1),
                          "ms": {n: [round(u, 4) for u in v] for n, v in t.items()},
                          "gbs": {n: round(size_of[n] / med[n] / 1e6, 1) for n in legs},
                          "speedup": {n: round(med["compose_" + n] / med[n], 2) for n in ours},
                          "us_per_frame": {"smooth_short": round(1e3 * med["smooth_short"] / Fs, 3),
                                           "compose_smooth_short": round(1e3 * med["compose_smooth_short"] / Fs, 3),
                                           "smooth": round(1e3 * med["smooth"] / F, 4)},
                          "spread": {n: round((max(v) - min(v)) / med[n], 3) for n, v in t.items()},
                          "copy_gbs": round(copy_tbs * 1e3, 1),
                          "kernels": [pv.time_kernel_name(op) for op in ("blur", "smooth", "freeze")]}), flush=True)
        del a, out, short, short_out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
