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

--fade: the timed crossfade of response changes (push_ir_fade), one line per shape, in four parts.  The plain path of
this build against another build of the library (--parent-lib, the parent commit's libclfft_amd.so) in one process, both
through the C ABI, in four alternating legs each, with two objects of the other build: every leg's median and worst
phase, so that the difference between the builds' means can be held against what one build's own legs, and its own two
objects, differ by.  A block of a fade (median, worst phase) against the composition it replaces: two NupconvMatrix
objects fed alike and the three torch operations of the mix.  The fade push itself (the response transforms and the
priming of the second set) beside a plain push, median of three.  And the state before and after the first fade,
against two objects.

    python tools/time_nupconv_matrix.py --fade [--parent-lib old/libclfft_amd.so] [--out profiles/nupconv_matrix_fade.txt]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import opencl_fft_amd as fa  # noqa: E402
from time_nupconv import leg_stats, other_build  # noqa: E402  (tools/time_nupconv.py: the A/B of Nupconv's fade)

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


class Raw:
    """a NupconvMatrix of one build of the library through its C ABI: what both builds of an A/B are called through"""

    def __init__(self, lib, cvs, pts0, pts1, I, O, stream):
        self.lib, self.h, self.s = lib, C.c_void_p(), stream
        assert lib.clfa_nupconv_matrix_create(C.byref(self.h), 0, cvs, pts0, pts1, I, O) == 0

    def push(self, h):
        assert self.lib.clfa_nupconv_matrix_push_ir_dev(self.h, h.data_ptr(), h.stride(1), self.s) == 0

    def push_fade(self, h, blocks):
        assert self.lib.clfa_nupconv_matrix_push_ir_fade_dev(self.h, h.data_ptr(), h.stride(1), blocks, self.s) == 0

    def run(self, out, x):
        assert self.lib.clfa_nupconv_matrix_process_dev(self.h, out.data_ptr(), out.stride(0), x.data_ptr(), x.stride(0), 1, self.s) == 0

    def position(self):
        return self.lib.clfa_nupconv_matrix_position(self.h)

    def state_mib(self):
        return round(self.lib.clfa_nupconv_matrix_state_bytes(self.h) / 2 ** 20, 1)

    def close(self):
        self.lib.clfa_nupconv_matrix_destroy(self.h)
        self.h = None


def fade_shape(cvs, pts0, pts1, I, O, periods, parent, new_position=0):
    from opencl_fft_amd import _lib
    m = pts1 // pts0
    n = periods * m
    s = torch.cuda.current_stream().cuda_stream
    h = torch.rand((O, I, cvs), device="cuda") - 0.5
    h2 = torch.rand((O, I, cvs), device="cuda") - 0.5
    x = torch.rand((I, pts0), device="cuda") - 0.5
    out = torch.empty((O, pts0), device="cuda")
    r = {"cvs": cvs, "pts0": pts0, "pts1": pts1, "inputs": I, "outputs": O, "periods": periods}

    def legs_of(run):
        return leg_stats(calls(run, n).reshape(periods, m) * 1e3)

    # the plain path: this build and the parent's in alternating legs
    # (two objects of the parent's: what two objects of ONE build differ by.  new_position: where this build's object
    # stands in the order of creation and of the first leg — an object's place shows in its times)
    roles = ["parent", "parent_2"] if parent is not None else []
    roles.insert(min(new_position, len(roles)), "new")
    r["order"] = roles
    builds = {}
    for k in roles:
        builds[k] = Raw(_lib.lib() if k == "new" else parent, cvs, pts0, pts1, I, O, s)
        builds[k].push(h)
    new = builds["new"]
    r["segments"] = [_lib.lib().clfa_nupconv_matrix_segments(new.h, k) for k in (0, 1)]
    for b in builds.values():
        calls(lambda: b.run(out, x), 2 * m)
    plain = {k: [] for k in builds}
    order = list(builds)
    for _ in range(4):                          # forwards, backwards, ...: no object always follows the same other
        for k in order:
            assert builds[k].position() % m == 0
            plain[k].append(legs_of(lambda: builds[k].run(out, x)))
        order.reverse()
    r["plain_us"] = plain
    if parent is not None:
        keys = ("median", "worst_phase")
        mean = {b: {k: float(np.mean([l[k] for l in plain[b]])) for k in keys} for b in plain}
        r["parent_leg_spread_us"] = {k: round(max(l[k] for l in plain["parent"]) - min(l[k] for l in plain["parent"]), 2) for k in keys}
        r["parent_object_spread_us"] = {k: round(abs(mean["parent"][k] - mean["parent_2"][k]), 2) for k in keys}
        r["new_minus_parent_us"] = {k: round(mean["new"][k] - (mean["parent"][k] + mean["parent_2"][k]) / 2, 2) for k in keys}
        builds.pop("parent").close()
        builds.pop("parent_2").close()
    # a block of a fade against the composition it replaces: two objects fed alike and the mix in three torch operations
    ca, cb = Raw(_lib.lib(), cvs, pts0, pts1, I, O, s), Raw(_lib.lib(), cvs, pts0, pts1, I, O, s)
    ca.push(h)
    cb.push(h2)
    ya, yb, d = torch.empty_like(out), torch.empty_like(out), torch.empty_like(out)
    g = (torch.arange(pts0, device="cuda", dtype=torch.float32) / float(n * pts0)).expand_as(out).contiguous()

    def composition():
        ca.run(ya, x)
        cb.run(yb, x)
        torch.sub(yb, ya, out=d)
        d.mul_(g)
        torch.add(ya, d, out=out)

    r["state_mib"] = {"before_the_first_fade": new.state_mib(), "two_objects": round(ca.state_mib() + cb.state_mib(), 1)}
    new.push_fade(h2, 2 * m)                    # warm-up: the first fade allocates the second set
    r["state_mib"]["after_the_first_fade"] = new.state_mib()
    calls(lambda: new.run(out, x), 2 * m)
    calls(composition, 2 * m)
    fade, comp = [], []
    for leg in range(2):
        assert new.position() % m == 0
        new.push_fade(h if leg % 2 == 0 else h2, n)
        fade.append(legs_of(lambda: new.run(out, x)))
        comp.append(legs_of(composition))
    r["fade_block_us"], r["composition_block_us"] = fade, comp
    r["fade_over_composition"] = {k: round(float(np.mean([l[k] for l in fade]) / np.mean([l[k] for l in comp])), 3)
                                  for k in ("median", "worst_phase")}
    ca.close()
    cb.close()
    # the push: a fade push (response transforms and priming; phases 0, 1, 2 of a period past the third) beside a plain one
    tf, tp = [], []
    for k in range(3):
        tf.append(calls(lambda: new.push_fade(h2 if k % 2 == 0 else h, 1), 1)[0])
        new.run(out, x)
    for k in range(3):
        tp.append(calls(lambda: new.push(h), 1)[0])
    r["push_ms"] = {"fade": round(float(np.median(tf)), 3), "plain": round(float(np.median(tp)), 3)}
    r["block_lasts_us_at_48k"] = round(pts0 / 48e3 * 1e6, 1)
    new.close()
    torch.cuda.synchronize()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fade", action="store_true", help="the timed crossfade: plain path A/B, fade block, fade push, state")
    ap.add_argument("--parent-lib", default=None, help="--fade: another build of libclfft_amd.so to hold the plain path against")
    ap.add_argument("--new-position", type=int, default=0, choices=(0, 1, 2),
                    help="--fade: this build's object is created first (0), between the parent's two (1) or last (2)")
    ap.add_argument("--periods", type=int, default=3)
    ap.add_argument("--cvs", type=int, default=1 << 18)
    ap.add_argument("--signal", type=int, default=256, help="head blocks of the whole-signal call")
    ap.add_argument("--leg-budget-s", type=float, default=20.0)
    ap.add_argument("--quick", action="store_true", help="without the 64 x 64 shapes")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    lines = [json.dumps({"device": fa.device_name(0), "how": __doc__.split("\n\n")[2 if a.fade else 0].replace("\n", " ")})]
    probe = {k: round(v, 3) for k, v in fa.bandwidth_probe(0, 1 << 30, 100).items()}
    lines.append(json.dumps({"bandwidth_probe_tb_s": probe}))
    print(lines[-1], flush=True)
    parent = other_build(a.parent_lib) if a.fade and a.parent_lib else None
    for pts0, pts1, I, O in SHAPES:
        if a.quick and I * O > 256:
            continue
        if a.fade:
            lines.append(json.dumps(fade_shape(a.cvs, pts0, pts1, I, O, a.periods, parent, a.new_position)))
        else:
            lines.append(json.dumps(shape(a.cvs, pts0, pts1, I, O, a.periods, a.signal, a.leg_budget_s)))
        print(lines[-1], flush=True)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
