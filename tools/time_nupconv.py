"""Non-uniformly partitioned convolution (Nupconv, pconv_nup.hip) against the only way to the same latency without it:
Clpconv(cvs, pts0, channels).process_device once per block.  Single-block calls on one stream, each between two device
events: mean, median and the worst phase (the median over the periods of the slowest of the m phases — what a live
stream must budget for), phase 0 (forward transform of a tail block) and phase m - 1 (its inverse) on their own.  The two
objects alternate in legs of --periods periods each (two legs; alternating period by period would put every phase-0 call
behind the other object's calls, on cold caches, and charge that to the phase).  Beside the times: the bytes a call must
read (the rings of both levels' slices / both whole rings), the rate they give, and the box's copy rate
(bandwidth_probe) to hold them against.  One line per shape records a whole-signal call of 1024 head blocks.

    python tools/time_nupconv.py [--periods 4] [--cvs 1048576] [--quick] [--out profiles/nupconv.txt]
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

SHAPES = [(64, 4096, 1), (64, 4096, 16), (64, 4096, 256), (256, 4096, 1), (256, 4096, 16), (256, 4096, 256)]


def nup_bytes(cvs, pts0, pts1):
    """ring bytes one head block reads per channel: the head's 2m partitions and n1 tail slices of pts0 bins, 8 bytes a
    bin, input and response rings"""
    return 16 * (2 * pts1 + (cvs - 2 * pts1) // pts1 * pts0)


def calls(fn, n):
    """device time of n consecutive calls, each between its own pair of events: ms"""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return np.array([a.elapsed_time(b) for a, b in ev])


def shape(cvs, pts0, pts1, channels, periods):
    m = pts1 // pts0
    s = torch.cuda.current_stream().cuda_stream
    h = torch.rand((channels, cvs), device="cuda") - 0.5
    x = torch.rand((channels, pts0), device="cuda") - 0.5
    out = torch.empty_like(x)
    nup = fa.Nupconv(0, cvs, pts0, pts1, channels=channels)
    assert nup.get_error() == 0, nup.get_log()
    assert nup.push_ir_device(h, s) == 0
    base = fa.Clpconv(0, cvs, pts0, channels=channels)
    assert base.get_cl_err() == 0 and base.push_ir_device(h, s) == 0
    del h

    def run_nup():
        assert nup.process_device(out, x, s) == 0

    def run_base():
        assert base.process_device(out, x, None, s) == 0

    # warm-up: two periods each, so that every phase's kernels are loaded and a tail block is being heard
    calls(run_nup, 2 * m)
    calls(run_base, 2 * m)
    tn, tb = [], []
    for _ in range(2):
        assert nup.position % m == 0
        tn.append(calls(run_nup, periods * m).reshape(periods, m))
        tb.append(calls(run_base, periods * m).reshape(periods, m))
    tn, tb = np.concatenate(tn) * 1e3, np.concatenate(tb) * 1e3      # (2 x periods) x phases, us
    by_phase = np.median(tn, axis=0)
    nb, bb = nup_bytes(cvs, pts0, pts1) * channels, 16 * (cvs // pts0 * pts0) * channels
    r = {"cvs": cvs, "pts0": pts0, "pts1": pts1, "channels": channels, "periods": periods,
         "nup_us": {"mean": round(float(tn.mean()), 2), "median": round(float(np.median(tn)), 2),
                    "worst_phase": round(float(by_phase.max()), 2), "worst_phase_index": int(by_phase.argmax()),
                    "phase_0": round(float(by_phase[0]), 2), "phase_m-1": round(float(by_phase[-1]), 2),
                    "max_single_call": round(float(tn.max()), 2)},
         "clpconv_us": {"mean": round(float(tb.mean()), 2), "median": round(float(np.median(tb)), 2),
                        "max_single_call": round(float(tb.max()), 2)},
         "computed_mb_per_call": {"nup": round(nb / 1e6, 3), "clpconv": round(bb / 1e6, 3)},
         "achieved_tb_s_at_median": {"nup": round(nb / np.median(tn) / 1e6, 3), "clpconv": round(bb / np.median(tb) / 1e6, 3)},
         "clpconv_kernel": base.kernel_name(),
         "state_mib": {"nup": round(nup.state_bytes() / 2 ** 20, 1), "clpconv": round(base.state_bytes() / 2 ** 20, 1)}}
    r["worst_phase_over_clpconv_median"] = round(r["nup_us"]["worst_phase"] / r["clpconv_us"]["median"], 3)
    del base
    # a whole signal: 1024 head blocks in one call (1024 / m period boundaries)
    K = 1024
    xs = torch.rand((channels, K * pts0), device="cuda") - 0.5
    os_ = torch.empty_like(xs)

    def run_signal():
        assert nup.process_device(os_, xs, s) == 0

    t = calls(run_signal, 4)[1:]
    r["signal_1024_blocks_ms"] = round(float(np.median(t)), 3)
    r["signal_us_per_block"] = round(float(np.median(t)) * 1e3 / K, 3)
    r["signal_boundaries"] = K // m
    del nup
    torch.cuda.synchronize()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--periods", type=int, default=4)
    ap.add_argument("--cvs", type=int, default=1 << 20)
    ap.add_argument("--quick", action="store_true", help="the one- and 16-channel shapes only")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.periods >= 3, "at least three periods"
    assert torch.cuda.is_available(), "needs a GPU"
    lines = [json.dumps({"device": fa.device_name(0), "how": __doc__.split("\n\n")[0].replace("\n", " ")})]
    probe = {k: round(v, 3) for k, v in fa.bandwidth_probe(0, 1 << 30, 100).items()}
    lines.append(json.dumps({"bandwidth_probe_tb_s": probe}))
    print(lines[-1], flush=True)
    for pts0, pts1, channels in SHAPES:
        if a.quick and channels > 16:
            continue
        lines.append(json.dumps(shape(a.cvs, pts0, pts1, channels, a.periods)))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
