"""Non-uniformly partitioned convolution matrix (NupconvMatrix, pconv_nupm.hip) against the two ways to the same result
without it: PconvMatrix(cvs, pts0, inputs, outputs), which reads every response whole in every block, and
Nupconv(channels = outputs * inputs) on expanded inputs followed by a torch sum over the inputs.  Single-block calls on one
stream, each between two device events: the median and the worst phase (the median over the periods of the slowest of the
m phases — what a live stream must budget for).  The three objects run in one process and alternate in legs of --periods
periods each (two legs each).  Beside the times: the bytes a block must read (responses and rings of both levels' slices /
the whole responses and rings), the rate they give, and the box's copy rate (bandwidth_probe) to hold them against.  One
figure per shape records a whole-signal call of --signal head blocks.  An object whose memory does not fit, or whose leg
would take longer than --leg-budget-s by its first calls, is left out and the line says so: no figure is extrapolated.

    python tools/time_nupconv_matrix.py [--periods 3] [--cvs 262144] [--quick] [--out profiles/nupconv_matrix.txt]
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

# pts0, pts1, inputs, outputs
SHAPES = [(64, 4096, 16, 2), (64, 4096, 4, 4), (64, 4096, 64, 64), (256, 4096, 16, 2), (256, 4096, 4, 4), (256, 4096, 64, 64)]


def calls(fn, n):
    """device time of n consecutive calls, each between its own pair of events: ms"""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return np.array([a.elapsed_time(b) for a, b in ev])


def stats(t):
    """t: periods x phases, us"""
    by_phase = np.median(t, axis=0)
    return {"median": round(float(np.median(t)), 2), "worst_phase": round(float(by_phase.max()), 2),
            "worst_phase_index": int(by_phase.argmax()), "max_single_call": round(float(t.max()), 2)}


def shape(cvs, pts0, pts1, I, O, periods, signal, leg_budget_s):
    m = pts1 // pts0
    n1 = (cvs - 2 * pts1) // pts1
    s = torch.cuda.current_stream().cuda_stream
    h = torch.rand((O, I, cvs), device="cuda") - 0.5
    x = torch.rand((I, pts0), device="cuda") - 0.5
    out = torch.empty((O, pts0), device="cuda")
    r = {"cvs": cvs, "pts0": pts0, "pts1": pts1, "inputs": I, "outputs": O, "periods": periods}
    runs, left_out = {}, {}

    nm = fa.NupconvMatrix(0, cvs, pts0, pts1, I, O)
    assert nm.get_error() == 0, nm.get_log()
    assert nm.push_ir_device(h, s) == 0
    r["segments"] = [nm.segments(0), nm.segments(1)]
    runs["nupconv_matrix"] = lambda: nm.process_device(out, x, s)

    pm = fa.PconvMatrix(0, cvs, pts0, I, O)
    if pm.get_error() == 0 and pm.push_ir_device(h, s) == 0:
        runs["pconv_matrix"] = lambda: pm.process_device(out, x, s)
    else:
        left_out["pconv_matrix"] = "creation or push failed: %d %s" % (pm.get_error(), pm.get_log())

    nu = fa.Nupconv(0, cvs, pts0, pts1, channels=O * I)
    xe, ye = x.repeat(O, 1), torch.empty((O * I, pts0), device="cuda")       # row o * I + i = input i
    if nu.get_error() == 0 and nu.push_ir_device(h.view(O * I, cvs), s) == 0:
        def run_nup():
            xe.view(O, I, pts0).copy_(x)                                      # the copies of the input ...
            e = nu.process_device(ye, xe, s)
            torch.sum(ye.view(O, I, pts0), dim=1, out=out)                    # ... and the reduction over them
            return e
        runs["nupconv_expanded"] = run_nup
    else:
        left_out["nupconv_expanded"] = "creation or push failed: %d %s" % (nu.get_error(), nu.get_log())
    del h

    # warm-up: two periods each, so that every phase's kernels are loaded and a tail block is being heard; an object
    # whose legs would not fit the budget is left out (its warm-up calls are all that was run of it)
    for k in list(runs):
        t = calls(lambda: runs[k]() == 0 or sys.exit("%s failed" % k), 2 * m)
        if float(t.mean()) * 1e-3 * periods * m * 2 > leg_budget_s:
            left_out[k] = "left out: %.0f us per call in the warm-up, two legs would take %.0f s" % (
                t.mean() * 1e3, t.mean() * 1e-3 * periods * m * 2)
            r.setdefault("warm_up_only_us", {})[k] = round(float(np.median(t)) * 1e3, 2)
            del runs[k]
    times = {k: [] for k in runs}
    for _ in range(2):
        for k in runs:
            assert nm.position % m == 0
            times[k].append(calls(runs[k], periods * m).reshape(periods, m))
    r["block_us"] = {k: stats(np.concatenate(v) * 1e3) for k, v in times.items()}
    if left_out:
        r["left_out"] = left_out
    # bytes a block must read, 8 per bin: the responses (O x I rows) and the input rings (I rows) of what the block walks
    per_row = {"nupconv_matrix": 8 * (2 * pts1 + n1 * pts0), "pconv_matrix": 8 * (cvs // pts0 * pts0)}
    mb = {"nupconv_matrix": per_row["nupconv_matrix"] * (O * I + I) / 1e6,
          "pconv_matrix": per_row["pconv_matrix"] * (O * I + I) / 1e6,
          "nupconv_expanded": per_row["nupconv_matrix"] * 2 * O * I / 1e6}
    r["computed_mb_per_block"] = {k: round(v, 3) for k, v in mb.items()}
    r["achieved_tb_s_at_median"] = {k: round(mb[k] / r["block_us"][k]["median"], 3) for k in r["block_us"]}
    r["state_mib"] = {"nupconv_matrix": round(nm.state_bytes() / 2 ** 20, 1), "pconv_matrix": round(pm.state_bytes() / 2 ** 20, 1),
                      "nupconv_expanded": round(nu.state_bytes() / 2 ** 20, 1)}
    del pm, nu
    # a whole signal: `signal` head blocks in one call
    xs = torch.rand((I, signal * pts0), device="cuda") - 0.5
    os_ = torch.empty((O, signal * pts0), device="cuda")
    t = calls(lambda: nm.process_device(os_, xs, s), 3)[1:]
    r["signal_blocks"] = signal
    r["signal_ms"] = round(float(np.median(t)), 3)
    r["signal_us_per_block"] = round(float(np.median(t)) * 1e3 / signal, 3)
    r["block_lasts_us_at_48k"] = round(pts0 / 48e3 * 1e6, 1)
    del nm
    torch.cuda.synchronize()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--periods", type=int, default=3)
    ap.add_argument("--cvs", type=int, default=1 << 18)
    ap.add_argument("--signal", type=int, default=256, help="head blocks of the whole-signal call")
    ap.add_argument("--leg-budget-s", type=float, default=20.0)
    ap.add_argument("--quick", action="store_true", help="without the 64 x 64 shapes")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    lines = [json.dumps({"device": fa.device_name(0), "how": __doc__.split("\n\n")[0].replace("\n", " ")})]
    probe = {k: round(v, 3) for k, v in fa.bandwidth_probe(0, 1 << 30, 100).items()}
    lines.append(json.dumps({"bandwidth_probe_tb_s": probe}))
    print(lines[-1], flush=True)
    for pts0, pts1, I, O in SHAPES:
        if a.quick and I * O > 256:
            continue
        lines.append(json.dumps(shape(a.cvs, pts0, pts1, I, O, a.periods, a.signal, a.leg_budget_s)))
        print(lines[-1], flush=True)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
