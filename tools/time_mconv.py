"""Convolution matrix (PconvMatrix, pconv_matrix.hip) against the torch composition a caller writes today: every input
copied O times, Clpconv(channels = O*I).process_blocks_device, a sum over the inputs.  Same stream, us per block, K = 64
and K = 1 blocks per call, and the state bytes of both routes.  --sweep also times the matrix under other tiles and
segment counts (CLFA_PCONV_MATRIX_TILE / CLFA_PCONV_MATRIX_SEGS, read at creation).

    python tools/time_mconv.py [--reps 10] [--sweep] [--out profiles/pconv_matrix_r07.txt]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for name, I, O, pts, taps in CASES:
        for K in (64, 1):
            r = case(name, I, O, pts, taps, K, args.reps, args.sweep)
            print(json.dumps(r), flush=True)
            lines.append(json.dumps(r))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# Convolution matrix against the Clpconv composition (tools/time_mconv.py, median of %d timed calls, "
                    "%s)\n" % (args.reps, fa.device_name(0)))
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
