"""The per-bin delay of Pvoc (pvoc_delay.hip) against the torch composition a caller writes without it.  16 channels x 2^22
samples, hop = size / 4, max_delay 64.  Three medians per leg, the legs interleaved; algorithmic GB/s counts the input
stream and the output once each.  One JSON line per size, with the copy figure of the same box (bandwidth_probe) beside it.

  no feedback  a constant delay of 16 frames, and a ramp of 0..64 frames over the bins, against torch.gather along the frame
               axis of the stream padded with 64 zero frames.  The padded stream and the index tensor are made once, outside
               the timed call: the composition is timed as the one gather.
  feedback     the ramp with g = 0.5, and the worst case d = 1 in every bin (every frame waits for the one before it, through
               memory).  The recurrence has no torch primitive: a Python loop over the frames (two gathers of the taps, the
               rule, one store), timed on a shorter stream (--loop-frames) beside the kernel on the same shorter stream;
               `us_per_frame` says what a frame costs each side.  The kernel is also timed on the whole stream.

    python tools/time_pvoc_delay.py [--sizes 256,2048,16384] [--channels 16] [--log2-samples 22] [--reps 10] [--loop-frames 256]
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

L = 64


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
        B = M + 1
        pv = fa.Pvoc(0, size, hop, sr, C)
        assert pv.get_error() == 0, pv.get_log()
        assert pv.delay_setup(L) == 0
        F = 1 + (samples - size) // hop
        Fs = min(args.loop_frames, F)
        g = torch.Generator(device=dev).manual_seed(size)
        a = torch.rand((C, F, B, 2), device=dev, generator=g) + 0.01
        out = torch.empty_like(a)
        short, short_out = a[:, :Fs].contiguous(), torch.empty((C, Fs, B, 2), device=dev)
        d_const = torch.full((B,), 16, dtype=torch.int32, device=dev)
        d_ramp = ((torch.arange(B, device=dev) * L) // M).to(torch.int32)
        d_one = torch.ones((B,), dtype=torch.int32, device=dev)
        half = torch.full((B,), 0.5, device=dev)
        padded = torch.nn.functional.pad(a, (0, 0, 0, 0, L, 0))
        short_padded = torch.nn.functional.pad(short, (0, 0, 0, 0, L, 0))
        frame_index = torch.arange(F, device=dev)

        def index_of(d):
            return (L + frame_index[:, None] - d[None, :].long())[None, :, :, None].expand(C, F, B, 2)

        idx_const, idx_ramp = index_of(d_const), index_of(d_ramp)

        def comp_loop(d):
            taps = (L - d.long())[None, None, :, None].expand(C, 1, B, 2)      # frame f reads row taps + f
            ys = torch.zeros((C, L + Fs, B, 2), device=dev)

            def run():
                for f in range(Fs):
                    x, y = torch.gather(short_padded, 1, taps + f)[:, 0], torch.gather(ys, 1, taps + f)[:, 0]
                    a2 = half * y[..., 0]
                    ys[:, L + f] = torch.stack([x[..., 0] + a2, torch.where(a2.abs() > x[..., 0].abs(), y[..., 1], x[..., 1])], dim=-1)
                return ys
            return run

        legs = {"const": lambda: pv.delay_device(a, out, d_const), "compose_const": lambda: torch.gather(padded, 1, idx_const),
                "ramp": lambda: pv.delay_device(a, out, d_ramp), "compose_ramp": lambda: torch.gather(padded, 1, idx_ramp),
                "fb_ramp_short": lambda: pv.delay_device(short, short_out, d_ramp, half), "compose_fb_ramp_short": comp_loop(d_ramp),
                "fb_d1_short": lambda: pv.delay_device(short, short_out, d_one, half), "compose_fb_d1_short": comp_loop(d_one),
                "fb_ramp": lambda: pv.delay_device(a, out, d_ramp, half),
                "fb_d1": lambda: pv.delay_device(a, out, d_one, half)}
        t = interleaved(legs, args.reps)
        med = {n: float(np.median(v)) for n, v in t.items()}
        nbytes = 2 * a.numel() * 4
        sbytes = 2 * short.numel() * 4
        size_of = {n: sbytes if n.endswith("_short") else nbytes for n in legs}
        ours = [n for n in legs if not n.startswith("compose_") and "compose_" + n in legs]
        frames_of = {n: Fs if n.endswith("_short") else F for n in legs if "fb_" in n}
        print(json.dumps({"size": size, "hop": hop, "channels": C, "frames": F, "loop_frames": Fs, "max_delay": L, "bytes": nbytes,
                          "lanes_fb": C * B,
                          "ms": {n: [round(u, 4) for u in v] for n, v in t.items()},
                          "gbs": {n: round(size_of[n] / med[n] / 1e6, 1) for n in legs},
                          "speedup": {n: round(med["compose_" + n] / med[n], 2) for n in ours},
                          "us_per_frame": {n: round(1e3 * med[n] / k, 4) for n, k in frames_of.items()},
                          "spread": {n: round((max(v) - min(v)) / med[n], 3) for n, v in t.items()},
                          "copy_gbs": round(copy_tbs * 1e3, 1),
                          "kernels": [pv.delay_kernel_name(fb) for fb in (False, True)]}), flush=True)
        del a, out, short, short_out, padded, short_padded, idx_const, idx_ramp
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
