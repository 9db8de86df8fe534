"""Convolution matrix (PconvMatrix, pconv_matrix.hip) against the torch composition a caller writes today: every input
copied O times, Clpconv(channels = O*I).process_blocks_device, a sum over the inputs.  Same stream, us per block, K = 64
and K = 1 blocks per call, and the state bytes of both routes.  --sweep also times the matrix under other tiles and
segment counts (CLFA_PCONV_MATRIX_TILE / CLFA_PCONV_MATRIX_SEGS, read at creation).  --fade measures the timed crossfade
(push_ir_fade_device) instead: a fade block against a steady block, against the composition a caller writes without it
(two PconvMatrix objects and torch.lerp with a precomputed ramp), the two-response MAC against two launches of the plain
one (CLFA_PCONV_MATRIX_FADE_MAC=two), and the fade push against a plain push; the legs of a comparison are interleaved and
repeated, and the spread of the repeats is printed with them.

    python tools/time_mconv.py [--reps 10] [--sweep] [--out profiles/pconv_matrix_r07.txt]
    python tools/time_mconv.py --fade [--reps 10] [--out profiles/pconv_matrix_fade_r10.txt]
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

CASES = [  # name, inputs, outputs, pts, taps
    ("16to2", 16, 2, 512, 96000),
    ("4x4", 4, 4, 1024, 144000),
    ("64x64", 64, 64, 256, 4096),
]
SWEEP = [(kt, segs) for kt in (4, 16) for segs in (4, 16, 64, 256)]


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


def matrix(cvs, pts, I, O, ir, env=None):
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        m = fa.PconvMatrix(0, cvs, pts, I, O)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    assert m.get_error() == 0, m.get_log()
    assert m.push_ir(ir) == 0
    return m


def case(name, I, O, pts, taps, K, reps, sweep):
    rng = np.random.default_rng(1)
    nparts = taps // pts
    ir = rng.random((O, I, nparts * pts), dtype=np.float32) - 0.5
    s = torch.cuda.current_stream().cuda_stream
    L = K * pts
    x = torch.rand((I, L), device="cuda") - 0.5
    out = torch.empty((O, L), device="cuda")
    m = matrix(taps, pts, I, O, ir)
    p = fa.Clpconv(0, taps, pts, channels=O * I)
    assert p.get_cl_err() == 0 and p.push_ir(ir.reshape(O * I, -1)) == 0
    xin = torch.empty((O * I, L), device="cuda")
    y = torch.empty((O * I, L), device="cuda")
    cout = torch.empty((O, L), device="cuda")

    def run_matrix(obj=m):
        assert obj.process_device(out, x, s) == 0

    def run_comp():
        xin.view(O, I, L).copy_(x.unsqueeze(0).expand(O, I, L))
        assert p.process_blocks_device(y, xin, None, s) == 0
        torch.sum(y.view(O, I, L), dim=1, out=cout)

    t_m, t_c = timed(run_matrix, reps), timed(run_comp, reps)
    r = {"case": name, "inputs": I, "outputs": O, "pts": pts, "nparts": nparts, "K": K,
         "matrix_us_per_block": round(t_m * 1e3 / K, 2), "composition_us_per_block": round(t_c * 1e3 / K, 2),
         "speedup": round(t_c / t_m, 2),
         "matrix_state_mib": round(m.state_bytes() / 2 ** 20, 1),
         "composition_state_mib": round(p.state_bytes() / 2 ** 20, 1),
         "matrix_workspace_mib": round(m.workspace_bytes() / 2 ** 20, 1),
         "composition_workspace_mib": round(p.blocks_workspace_bytes() / 2 ** 20, 1)}
    if sweep:
        r["sweep_us_per_block"] = {}
        for kt, segs in SWEEP:
            if segs > I * nparts:
                continue
            q = matrix(taps, pts, I, O, ir, {"CLFA_PCONV_MATRIX_TILE": str(kt), "CLFA_PCONV_MATRIX_SEGS": str(segs)})
            r["sweep_us_per_block"]["kt%d_s%d" % (kt, segs)] = round(timed(lambda: run_matrix(q), reps) * 1e3 / K, 2)
            del q
    del m, p
    torch.cuda.synchronize()
    return r


def interleaved(fns, reps, legs=3, warm=2):
    """{name: [median ms of each leg]}: per leg `reps` rounds, each round one timed call of every function in turn"""
    for _ in range(warm):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = {k: [] for k in fns}
    for _ in range(legs):
        ts = {k: [] for k in fns}
        for _ in range(reps):
            for k, fn in fns.items():
                a.record()
                fn()
                b.record()
                b.synchronize()
                ts[k].append(a.elapsed_time(b))
        for k in fns:
            out[k].append(float(np.median(ts[k])))
    return out


def fade_case(name, I, O, pts, taps, K, reps):
    rng = np.random.default_rng(1)
    nparts = taps // pts
    ha = rng.random((O, I, nparts * pts), dtype=np.float32) - 0.5
    hb = torch.from_numpy(rng.random((O, I, nparts * pts), dtype=np.float32) - 0.5).cuda()
    s = torch.cuda.current_stream().cuda_stream
    L = K * pts
    x = torch.rand((I, L), device="cuda") - 0.5
    out, oa, ob = (torch.empty((O, L), device="cuda") for _ in range(3))
    long_fade = 1 << 20   # blocks: every timed call lies inside the fade
    steady = matrix(taps, pts, I, O, ha)
    fade = matrix(taps, pts, I, O, ha)
    two = matrix(taps, pts, I, O, ha, {"CLFA_PCONV_MATRIX_FADE_MAC": "two"})
    ca, cb = matrix(taps, pts, I, O, ha), matrix(taps, pts, I, O, ha)
    assert cb.push_ir_device(hb) == 0
    for m in (fade, two):
        assert m.process_device(out, x, s) == 0
        assert m.push_ir_fade_device(hb, long_fade, s) == 0
    ramp = (torch.arange(L, device="cuda", dtype=torch.float32) / float(L)).expand(O, L).contiguous()

    def run(m):
        return lambda: m.process_device(out, x, s)

    def run_comp():
        ca.process_device(oa, x, s)
        cb.process_device(ob, x, s)
        torch.lerp(oa, ob, ramp, out=out)

    t = interleaved({"steady": run(steady), "fade": run(fade), "fade_two_mac": run(two), "composition": run_comp}, reps)
    # the pushes: a one-block fade is finished by an untimed block between two of them
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    pusher = matrix(taps, pts, I, O, ha)
    x1, o1 = x[:, :pts].contiguous(), torch.empty((O, pts), device="cuda")
    tp = {"push_plain": [], "push_fade": []}
    for r in range(reps + 2):
        for k in tp:
            a.record()
            rc = pusher.push_ir_device(hb, s) if k == "push_plain" else pusher.push_ir_fade_device(hb, 1, s)
            b.record()
            b.synchronize()
            assert rc == 0
            if r >= 2:
                tp[k].append(a.elapsed_time(b))
            assert pusher.process_device(o1, x1, s) == 0
    us = lambda v: [round(q * 1e3 / K, 2) for q in v]
    spread = lambda v: round((max(v) - min(v)) * 1e3 / K, 2)
    r = {"case": name, "inputs": I, "outputs": O, "pts": pts, "nparts": nparts, "K": K}
    for k, v in t.items():
        r[k + "_us_per_block"] = us(v)
    r["spread_us_per_block"] = max(spread(v) for v in t.values())
    r["fade_over_steady"] = round(float(np.median(t["fade"]) / np.median(t["steady"])), 2)
    r["composition_over_fade"] = round(float(np.median(t["composition"]) / np.median(t["fade"])), 2)
    r["two_mac_over_fade"] = round(float(np.median(t["fade_two_mac"]) / np.median(t["fade"])), 2)
    r["push_plain_us"] = round(float(np.median(tp["push_plain"])) * 1e3, 1)
    r["push_fade_us"] = round(float(np.median(tp["push_fade"])) * 1e3, 1)
    r["fade_state_mib"] = round(fade.state_bytes() / 2 ** 20, 1)
    r["two_objects_state_mib"] = round((ca.state_bytes() + cb.state_bytes()) / 2 ** 20, 1)
    r["fade_workspace_mib"] = round(fade.workspace_bytes() / 2 ** 20, 1)
    r["two_objects_workspace_mib"] = round((ca.workspace_bytes() + cb.workspace_bytes()) / 2 ** 20, 1)
    del steady, fade, two, ca, cb, pusher
    torch.cuda.synchronize()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--fade", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for name, I, O, pts, taps in CASES:
        for K in (64, 1):
            r = fade_case(name, I, O, pts, taps, K, args.reps) if args.fade else case(name, I, O, pts, taps, K, args.reps, args.sweep)
            print(json.dumps(r), flush=True)
            lines.append(json.dumps(r))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            what = ("Timed crossfade of the convolution matrix: per leg the median of %d interleaved calls, three legs each"
                    if args.fade else "Convolution matrix against the Clpconv composition (tools/time_mconv.py, median of %d timed calls")
            f.write("# " + what % args.reps + ", %s)\n" % fa.device_name(0))
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
