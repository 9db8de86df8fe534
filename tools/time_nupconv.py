"""Non-uniformly partitioned convolution (Nupconv, pconv_nup.hip) against the only way to the same latency without it:
Clpconv(cvs, pts0, channels).process_device once per block.  Single-block calls on one stream, each between two device
events: mean, median and the worst phase (the median over the periods of the slowest of the m phases — what a live
stream must budget for), phase 0 (forward transform of a tail block) and phase m - 1 (its inverse) on their own.  The two
objects alternate in legs of --periods periods each (two legs; alternating period by period would put every phase-0 call
behind the other object's calls, on cold caches, and charge that to the phase).  Beside the times: the bytes a call must
read (the rings of both levels' slices / both whole rings), the rate they give, and the box's copy rate
(bandwidth_probe) to hold them against.  One line per shape records a whole-signal call of 1024 head blocks.

    python tools/time_nupconv.py [--periods 4] [--cvs 1048576] [--quick] [--out profiles/nupconv.txt]

--fade: the timed crossfade of response changes (push_ir_fade), one line per shape, in three parts.  The plain path of
this build against another build of the library (--parent-lib, the parent commit's libclfft_amd.so) in one process, both
through the C ABI, in four alternating legs each, with two objects of the other build: every leg's median and worst
phase, so that the difference between the builds' means can be held against what one build's own legs, and its own two
objects, differ by.  A block of a fade (median, worst phase) against the
composition it replaces: two Nupconv objects fed alike and the three torch operations of the mix.  And the fade push
itself (the response transforms and the priming of the second path) beside a plain push.

    python tools/time_nupconv.py --fade [--parent-lib old/libclfft_amd.so] [--out profiles/nupconv_fade.txt]

--tv: the time-varying second input (process_tv_device), one line per shape.  Single-block calls in two alternating legs
of --periods periods each (at least 4), every time-varying leg begun at the start of a response period, so that its first
two periods are the blocks that rewrite a head partition (a < 2m) and the rest those that do not: median and worst phase
of each kind.  Each is held against the same object's plain block (the cost of the second input) and against the only
other way to a time-varying response at this latency, Clpconv(cvs, pts0).process_device(out, x, w), in the same process.
A whole-signal call of 1024 head blocks from the start of a response period is held against
Clpconv.process_blocks_device with two inputs.

    python tools/time_nupconv.py --tv [--out profiles/nupconv_tv.txt]
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


def tv_shape(cvs, pts0, pts1, channels, periods):
    m = pts1 // pts0
    n = periods * m
    s = torch.cuda.current_stream().cuda_stream
    h = torch.rand((channels, cvs), device="cuda") - 0.5
    x = torch.rand((channels, pts0), device="cuda") - 0.5
    w = torch.rand((channels, pts0), device="cuda") - 0.5
    out = torch.empty_like(x)
    K = 1024
    xs = torch.rand((channels, K * pts0), device="cuda") - 0.5
    ws = torch.rand((channels, K * pts0), device="cuda") - 0.5
    os_ = torch.empty_like(xs)
    nup = fa.Nupconv(0, cvs, pts0, pts1, channels=channels)
    assert nup.get_error() == 0, nup.get_log()
    assert nup.push_ir_device(h, s) == 0
    base = fa.Clpconv(0, cvs, pts0, channels=channels)
    assert base.get_cl_err() == 0 and base.push_ir_device(h, s) == 0
    del h
    R0 = nup.tv_period
    assert R0 % m == 0 and n > 2 * m

    def to_period_start():
        """plain calls of many blocks up to the next multiple of R0"""
        left = (-nup.position) % R0
        while left:
            k = min(left, K)
            assert nup.process_device(os_[:, :k * pts0], xs[:, :k * pts0], s) == 0
            left -= k

    def run_tv():
        assert nup.process_tv_device(out, x, w, s) == 0

    def run_plain():
        assert nup.process_device(out, x, s) == 0

    def run_base():
        assert base.process_device(out, x, w, s) == 0

    for f in (run_plain, run_tv, run_base):
        calls(f, 2 * m)
    tv, plain, tb = [], [], []
    for _ in range(2):
        to_period_start()
        tv.append(calls(run_tv, n).reshape(periods, m))
        assert nup.position % m == 0
        plain.append(calls(run_plain, n).reshape(periods, m))
        tb.append(calls(run_base, n).reshape(periods, m))
    rewrite = np.concatenate([t[:2] for t in tv]) * 1e3        # a < 2m: the first two periods of a response period
    static = np.concatenate([t[2:] for t in tv]) * 1e3
    plain, tb = np.concatenate(plain) * 1e3, np.concatenate(tb) * 1e3

    def stats(t):
        by_phase = np.median(t, axis=0)
        return {"median": round(float(np.median(t)), 2), "worst_phase": round(float(by_phase.max()), 2),
                "worst_phase_index": int(by_phase.argmax()), "max_single_call": round(float(t.max()), 2)}

    r = {"cvs": cvs, "pts0": pts0, "pts1": pts1, "channels": channels, "periods": periods, "tv_period_blocks": R0,
         "tv_rewrite_us": stats(rewrite), "tv_static_us": stats(static), "plain_us": stats(plain),
         "clpconv_tv_us": {"median": round(float(np.median(tb)), 2), "max_single_call": round(float(tb.max()), 2)},
         "clpconv_kernel": base.kernel_name()}
    worst = max(r["tv_rewrite_us"]["worst_phase"], r["tv_static_us"]["worst_phase"])
    r["tv_worst_phase_over_plain_worst_phase"] = round(worst / r["plain_us"]["worst_phase"], 3)
    r["tv_worst_phase_over_clpconv_tv_median"] = round(worst / r["clpconv_tv_us"]["median"], 3)
    # a whole signal of 1024 head blocks from the start of a response period, against Clpconv's blocks route with two inputs
    def run_signal():
        to_period_start()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        assert nup.process_tv_device(os_, xs, ws, s) == 0
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    t = [run_signal() for _ in range(4)][1:]
    tbs = calls(lambda: base.process_blocks_device(os_, xs, ws, s), 4)[1:]
    r["signal_1024_blocks_ms"] = {"nup_tv": round(float(np.median(t)), 3), "clpconv_tv_blocks": round(float(np.median(tbs)), 3)}
    r["signal_nup_over_clpconv"] = round(float(np.median(t) / np.median(tbs)), 3)
    r["clpconv_blocks_kernel"] = base.blocks_kernel_name()
    r["state_mib"] = {"nup": round(nup.state_bytes() / 2 ** 20, 1), "clpconv": round(base.state_bytes() / 2 ** 20, 1)}
    del nup, base
    torch.cuda.synchronize()
    return r


class Raw:
    """a Nupconv of one build of the library through its C ABI: what both builds of an A/B are called through"""

    def __init__(self, lib, cvs, pts0, pts1, channels, stream):
        self.lib, self.h, self.s = lib, C.c_void_p(), stream
        assert lib.clfa_nupconv_create(C.byref(self.h), 0, cvs, pts0, pts1, channels) == 0

    def push(self, h):
        assert self.lib.clfa_nupconv_push_ir_dev(self.h, h.data_ptr(), h.stride(0), self.s) == 0

    def push_fade(self, h, blocks):
        assert self.lib.clfa_nupconv_push_ir_fade_dev(self.h, h.data_ptr(), h.stride(0), blocks, self.s) == 0

    def run(self, out, x):
        assert self.lib.clfa_nupconv_process_dev(self.h, out.data_ptr(), out.stride(0), x.data_ptr(), x.stride(0), 1, self.s) == 0

    def position(self):
        return self.lib.clfa_nupconv_position(self.h)

    def close(self):
        self.lib.clfa_nupconv_destroy(self.h)
        self.h = None


def other_build(path):
    """another build of the library, its entry points typed like this one's (those it lacks are simply absent)"""
    from opencl_fft_amd import _lib
    lib = C.CDLL(path)
    for name, res, args in _lib.SYMBOLS:
        if hasattr(lib, name):
            f = getattr(lib, name)
            f.restype, f.argtypes = res, args
    return lib


def leg_stats(t):
    """t: periods x phases, us -> the leg's median and worst phase (the slowest of the phases' medians over the periods)"""
    by_phase = np.median(t, axis=0)
    return {"median": round(float(np.median(t)), 2), "worst_phase": round(float(by_phase.max()), 2),
            "worst_phase_index": int(by_phase.argmax())}


def fade_shape(cvs, pts0, pts1, channels, periods, parent):
    from opencl_fft_amd import _lib
    m = pts1 // pts0
    n = periods * m
    s = torch.cuda.current_stream().cuda_stream
    h = torch.rand((channels, cvs), device="cuda") - 0.5
    h2 = torch.rand((channels, cvs), device="cuda") - 0.5
    x = torch.rand((channels, pts0), device="cuda") - 0.5
    out = torch.empty_like(x)
    r = {"cvs": cvs, "pts0": pts0, "pts1": pts1, "channels": channels, "periods": periods}

    def legs_of(run):
        return leg_stats(calls(run, n).reshape(periods, m) * 1e3)

    # the plain path: this build and the parent's in alternating legs
    new = Raw(_lib.lib(), cvs, pts0, pts1, channels, s)
    new.push(h)
    builds = {"new": new}
    if parent is not None:                      # two objects of the parent's: what two objects of ONE build differ by
        for k in ("parent", "parent_2"):
            builds[k] = Raw(parent, cvs, pts0, pts1, channels, s)
            builds[k].push(h)
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
    ca, cb = Raw(_lib.lib(), cvs, pts0, pts1, channels, s), Raw(_lib.lib(), cvs, pts0, pts1, channels, s)
    ca.push(h)
    cb.push(h2)
    ya, yb, d = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    g = (torch.arange(pts0, device="cuda", dtype=torch.float32) / float(n * pts0)).expand_as(x).contiguous()

    def composition():
        ca.run(ya, x)
        cb.run(yb, x)
        torch.sub(yb, ya, out=d)
        d.mul_(g)
        torch.add(ya, d, out=out)

    new.push_fade(h2, 2 * m)                    # warm-up: the first fade allocates the second set
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
    r["state_mib_with_second_set"] = round(_lib.lib().clfa_nupconv_state_bytes(new.h) / 2 ** 20, 1)
    new.close()
    torch.cuda.synchronize()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--periods", type=int, default=4)
    ap.add_argument("--cvs", type=int, default=1 << 20)
    ap.add_argument("--quick", action="store_true", help="the one- and 16-channel shapes only")
    ap.add_argument("--out", default=None)
    ap.add_argument("--fade", action="store_true", help="the timed crossfade: plain path A/B, fade block, fade push")
    ap.add_argument("--tv", action="store_true", help="the time-varying second input against the plain block and Clpconv")
    ap.add_argument("--parent-lib", default=None, help="--fade: another build of libclfft_amd.so to hold the plain path against")
    a = ap.parse_args()
    assert a.periods >= 3, "at least three periods"
    assert torch.cuda.is_available(), "needs a GPU"
    assert not a.tv or a.periods >= 4, "--tv: at least four periods (two of each kind of block)"
    lines = [json.dumps({"device": fa.device_name(0), "how": __doc__.split("\n\n")[4 if a.tv else 2 if a.fade else 0].replace("\n", " ")})]
    probe = {k: round(v, 3) for k, v in fa.bandwidth_probe(0, 1 << 30, 100).items()}
    lines.append(json.dumps({"bandwidth_probe_tb_s": probe}))
    print(lines[-1], flush=True)
    parent = other_build(a.parent_lib) if a.fade and a.parent_lib else None
    for pts0, pts1, channels in SHAPES:
        if a.quick and channels > 16:
            continue
        if a.tv:
            lines.append(json.dumps(tv_shape(a.cvs, pts0, pts1, channels, a.periods)))
        elif a.fade:
            lines.append(json.dumps(fade_shape(a.cvs, pts0, pts1, channels, a.periods, parent)))
        else:
            lines.append(json.dumps(shape(a.cvs, pts0, pts1, channels, a.periods)))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
