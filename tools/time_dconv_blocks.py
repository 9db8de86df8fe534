"""Multi-block, multi-channel direct convolution (Cldconv.process_blocks_device, dconv_blocks.hip) against the loop a
caller writes without it: one process_device call per block on the same stream — for one channel the single-block
route of a one-channel object (k_dconv_block), for C channels C one-channel objects.  The two legs are interleaved and
each reports three medians (us per block); the last scenario also reports the fraction of the fp32 multiply-add peak
(157.3 TFLOP/s, 2 FLOP per tap and output).  Prints one JSON line per scenario.

    python tools/time_dconv_blocks.py [--reps 5] [--out profiles/dconv_blocks_r11.txt]
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

PEAK_FP32 = 157.3e12   # FLOP/s, vector fp32
SCENARIOS = [  # name, channels, irsize, vsize, nblocks
    ("1ch_1024x64", 1, 1024, 64, 256),
    ("64ch_1024x64", 64, 1024, 64, 256),
    ("1ch_96000x64", 1, 96000, 64, 256),
    ("16ch_256_1Msamples", 16, 256, 1024, 1024),
]


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


def scenario(name, ch, irsize, vsize, nb, reps):
    rng = np.random.default_rng(1)
    ir = (rng.random((ch, irsize), dtype=np.float32) - 0.5) / np.float32(np.sqrt(irsize))
    d = fa.Cldconv(0, irsize, vsize, channels=ch)
    assert d.get_cl_err() == 0 and d.push_ir(ir if ch > 1 else ir[0]) == 0
    singles = [fa.Cldconv(0, irsize, vsize) for _ in range(ch)]
    for c, o in enumerate(singles):
        assert o.get_cl_err() == 0 and o.push_ir(ir[c]) == 0
    L = nb * vsize
    a = torch.rand((ch, L), device="cuda") - 0.5
    out = torch.empty_like(a)
    # the loop's blocks, gathered once outside the timing (a caller holding block-major data pays nothing for it)
    blk_a = [[a[c, j * vsize:(j + 1) * vsize].contiguous() for j in range(nb)] for c in range(ch)]
    blk_o = [[torch.empty(vsize, device="cuda") for _ in range(nb)] for c in range(ch)]
    s = torch.cuda.current_stream().cuda_stream

    def loop():
        for j in range(nb):
            for c in range(ch):
                assert singles[c].process_device(blk_o[c][j], blk_a[c][j], None, s) == 0

    def blocks():
        assert d.process_blocks_device(out, a, None, s) == 0

    loop()
    blocks()
    torch.cuda.synchronize()
    t_loop, t_blocks = [], []
    for _ in range(3):   # interleaved legs
        t_loop.append(median_ms(loop, reps) * 1e3 / nb)
        t_blocks.append(median_ms(blocks, reps) * 1e3 / nb)
    spread = max(max(t_loop) - min(t_loop), max(t_blocks) - min(t_blocks))
    best = float(np.median(t_blocks))
    r = {"scenario": name, "channels": ch, "irsize": irsize, "vsize": vsize, "nblocks": nb,
         "blocks_kernel": d.blocks_kernel_name(),
         "loop_us_per_block": [round(t, 3) for t in t_loop], "blocks_us_per_block": [round(t, 3) for t in t_blocks],
         "speedup": round(float(np.median(t_loop)) / best, 2),
         "faster_by_more_than_the_spread": bool(min(t_loop) - max(t_blocks) > spread),
         "fp32_fma_peak_fraction": round(2.0 * ch * irsize * vsize / (best * 1e-6) / PEAK_FP32, 4),
         "workspace_mib": round(d.blocks_workspace_bytes() / 2 ** 20, 1)}
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="run one scenario by name")
    args = ap.parse_args()
    lines = []
    for name, ch, irsize, vsize, nb in SCENARIOS:
        if args.only and args.only != name:
            continue
        r = scenario(name, ch, irsize, vsize, nb, args.reps)
        print(json.dumps(r), flush=True)
        lines.append(json.dumps(r))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# Multi-block direct convolution against the single-block loop (tools/time_dconv_blocks.py: legs interleaved, "
                    "three medians of %d timed calls each, us per block, %s)\n" % (args.reps, fa.device_name(0)))
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
