"""Multi-block partitioned convolution (Clpconv.process_blocks_device, pconv_blocks.hip) against the loop a caller writes
today: one process_device call per block on the same stream.  Two shapes: config 4 (256 channels, pts 1024, 94
partitions, 64 blocks per call) and a single instance (1 channel, pts 512, 128 partitions, 256 blocks per call), static
and time-varying.  Prints one JSON line per case; rt48k = real-time ratio at 48 kHz (seconds of
audio per second of GPU time, every channel at once, the figure DESIGN.md quotes for config 4).

    python tools/time_pconv_blocks.py [--reps 10] [--out profiles/pconv_blocks_r06.txt]
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

CASES = [  # name, channels, pts, nparts, nblocks
    ("config4", 256, 1024, 94, 64),
    ("single", 1, 512, 128, 256),
]


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))   # ms


def case(name, ch, pts, nparts, nb, tv, reps):
    rng = np.random.default_rng(1)
    ir = rng.random((ch, pts * nparts), dtype=np.float32) - 0.5
    p = fa.Clpconv(0, pts * nparts, pts, channels=ch)
    assert p.get_cl_err() == 0 and p.push_ir(ir) == 0
    L = nb * pts
    a = torch.rand((ch, L), device="cuda") - 0.5
    b = torch.rand((ch, L), device="cuda") - 0.5 if tv else None
    out = torch.empty_like(a)
    # the loop's blocks, gathered once outside the timing (a caller holding block-major data pays nothing for it)
    blk_a = [a[:, j * pts:(j + 1) * pts].contiguous() for j in range(nb)]
    blk_b = [b[:, j * pts:(j + 1) * pts].contiguous() for j in range(nb)] if tv else [None] * nb
    blk_o = [torch.empty((ch, pts), device="cuda") for _ in range(nb)]
    s = torch.cuda.current_stream().cuda_stream

    def loop():
        for j in range(nb):
            assert p.process_device(blk_o[j], blk_a[j], blk_b[j], s) == 0

    def blocks():
        assert p.process_blocks_device(out, a, b, s) == 0

    t_loop, t_blocks = timed(loop, reps), timed(blocks, reps)
    per_loop, per_blocks = t_loop * 1e3 / nb, t_blocks * 1e3 / nb   # us per block
    audio_s = pts / 48000.0
    return {"case": name, "tv": tv, "channels": ch, "pts": pts, "nparts": nparts, "nblocks": nb,
            "single_kernel": p.kernel_name(), "blocks_kernel": p.blocks_kernel_name(),
            "loop_us_per_block": round(per_loop, 2), "blocks_us_per_block": round(per_blocks, 2),
            "speedup": round(per_loop / per_blocks, 2),
            "rt48k_loop": round(audio_s * 1e6 / per_loop, 1), "rt48k_blocks": round(audio_s * 1e6 / per_blocks, 1),
            "workspace_mib": round(p.blocks_workspace_bytes() / 2 ** 20, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for name, ch, pts, nparts, nb in CASES:
        for tv in (False, True):
            r = case(name, ch, pts, nparts, nb, tv, args.reps)
            print(json.dumps(r), flush=True)
            lines.append(json.dumps(r))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# Multi-block partitioned convolution against the single-block loop (tools/time_pconv_blocks.py, median of "
                    "%d timed calls, %s)\n" % (args.reps, fa.device_name(0)))
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
