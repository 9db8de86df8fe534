"""dev tool: how evenly the workgroups of the resident n = 65536 kernel finish (clfa_fft_balance_record / _read): per launch
the spread of the exit stamps, max - mean, as a fraction of the launch — what a perfect assignment could still gain — per
workgroup and per XCD (workgroup index % 8), and how many transforms each XCD's workgroups ran.  4096 transforms in place
on random data, directions alternating, launches taken after the settle steps.
usage: python tools/res16_balance.py [batch [launches]]      (CLFA_RES16_STATIC=1: the static assignment)"""
import os
import statistics
import sys
sys.path.insert(0, ".")
import numpy as np
import torch
import opencl_fft_amd as fa

batch = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
launches = int(sys.argv[2]) if len(sys.argv) > 2 else 12
plans = (fa.Clcfft(0, 65536, True), fa.Clcfft(0, 65536, False))
d = torch.rand((batch, 65536, 2), device="cuda") * 2 - 1
s = torch.cuda.current_stream().cuda_stream
for k in range(40):                       # settle: clocks and caches as in a long run
    plans[k & 1].exec_device(d, batch, s)
torch.cuda.synchronize()
for p in plans:
    assert p.balance_record(True) == 0
print("assignment: %s, batch %d" % ("static (CLFA_RES16_STATIC)" if os.environ.get("CLFA_RES16_STATIC") else "library default", batch))
wg, xc = [], []
for k in range(launches):
    p = plans[k & 1]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    p.exec_device(d, batch, s)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)
    rec = p.balance_read()
    t = rec["stamp"].astype(np.float64) / 100.0          # us (100 MHz)
    per_x = np.array([t[rec["xcd"] == x].mean() for x in range(8)])
    cnt_x = [int(rec["count"][rec["xcd"] == x].sum()) for x in range(8)]
    f_wg, f_x = (t.max() - t.mean()) / (ms * 1e3), (per_x.max() - per_x.mean()) / (ms * 1e3)
    wg.append(f_wg)
    xc.append(f_x)
    print("launch %2d %s %.4f ms  exit stamps: max - mean %6.1f us = %.4f of the launch, max - min %6.1f us; XCD means: max - mean "
          "%6.1f us = %.4f, late XCD %d; transforms per XCD %s, per workgroup %d..%d"
          % (k, "fwd" if k % 2 == 0 else "inv", ms, t.max() - t.mean(), f_wg, t.max() - t.min(), per_x.max() - per_x.mean(), f_x,
             int(per_x.argmax()), cnt_x, rec["count"].min(), rec["count"].max()))
print("max - mean of the exit stamps over the launch: per workgroup median %.4f (%.4f .. %.4f), per XCD median %.4f (%.4f .. %.4f)"
      % (statistics.median(wg), min(wg), max(wg), statistics.median(xc), min(xc), max(xc)))
del plans, p   # before the interpreter takes the library apart
