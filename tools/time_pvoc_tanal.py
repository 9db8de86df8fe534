"""The analysis of a stored signal at given time points (Pvoc.tanal_device, tanal_kernels.hip: k_pvoc_tanal) against
(a) the composition that defines it — the slices x_c[s - hop .. s + size) gathered by a torch index (the index is made
    outside the timed region; the gather, Stft.analyze_device, Pvoc.analyze_device and the copy of frame 1 are timed), in
    chunks of about 1 GiB of gathered samples — whose bits it must give (checked here at every shape), and
(b) for orientation only, today's route to another speed: Stft.analyze_device + Pvoc.analyze_device over the whole signal
    and Pvoc.read_device at the positions starts / hop, which computes something else (a blend of two grid frames).
16 channels x 2^22 samples, Hann window, hop = size / 4, time stretches by 1, 2 and 8.  Three medians per leg, the legs
interleaved; algorithmic GB/s counts the signal once and the frames once.  One JSON line per size and factor, with the
copy figure of the same box (bandwidth_probe) beside it.

    python tools/time_pvoc_tanal.py [--sizes 256,2048,16384] [--factors 1,2,8] [--channels 16] [--log2-samples 22] [--reps 5]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,2048,16384")
    ap.add_argument("--factors", default="1,2,8")
    ap.add_argument("--channels", type=int, default=16)
    ap.add_argument("--log2-samples", type=int, default=22)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sr", type=float, default=48000.0)
    args = ap.parse_args()
    C, samples, sr = args.channels, 1 << args.log2_samples, args.sr
    dev = "cuda:0"
    copy_tbs = fa.bandwidth_probe(0)["copy"]
    x = torch.rand((C, samples), device=dev) * 2 - 1
    for size in [int(s) for s in args.sizes.split(",")]:
        hop, M, L = size // 4, size // 2, size + size // 4
        w = torch.from_numpy((0.5 - 0.5 * np.cos(2 * np.pi * np.arange(size) / size)).astype(np.float32)).to(dev)
        pv = fa.Pvoc(0, size, hop, sr, C)
        st = fa.Stft(0, size, hop, window=w)
        assert pv.get_error() == 0 and st.get_error() == 0
        xpad = torch.zeros((C, samples + 2 * L), device=dev)        # (a)'s zeros outside the rows
        xpad[:, L:L + samples] = x
        Fgrid = st.frames(samples)
        spec = torch.empty((C, Fgrid, M), dtype=torch.complex64, device=dev)     # (b)'s spectra and frames on the hop grid
        grid = torch.empty((C, Fgrid, M + 1, 2), device=dev)
        for factor in [float(f) for f in args.factors.split(",")]:
            starts_h = fa.Pvoc.stretch_starts(samples, hop, factor)
            Fout = starts_h.size
            starts = torch.from_numpy(starts_h).to(dev)
            out = torch.empty((C, Fout, M + 1, 2), device=dev)
            out_a, out_b = torch.empty_like(out), torch.empty_like(out)
            # (a): the index of every slice, and per chunk of frames the buffers and a fresh Pvoc of C x chunk channels
            index = (starts.long() - hop + L)[:, None] + torch.arange(L, device=dev)
            step = max(1, min(Fout, (1 << 28) // (C * L)))
            chunks = [(f0, min(Fout, f0 + step)) for f0 in range(0, Fout, step)]
            objs = {n: fa.Pvoc(0, size, hop, sr, C * n) for n in {f1 - f0 for f0, f1 in chunks}}
            assert all(o.get_error() == 0 for o in objs.values())
            cspec = torch.empty((C * step, 2, M), dtype=torch.complex64, device=dev)
            cfr = torch.empty((C * step, 2, M + 1, 2), device=dev)

            def compose():
                for f0, f1 in chunks:
                    n = f1 - f0
                    sl = xpad[:, index[f0:f1]].reshape(C * n, L)
                    assert st.analyze_device(sl, cspec[:C * n]) == 0
                    assert objs[n].analyze_device(cspec[:C * n], cfr[:C * n]) == 0
                    out_a[:, f0:f1] = cfr[:C * n, 1].reshape(C, n, M + 1, 2)

            pos = (starts.float() / hop).contiguous()

            def read_route():
                assert st.analyze_device(x, spec) == 0
                assert pv.analyze_device(spec, grid) == 0
                assert pv.read_device(grid, pos, out_b) == 0

            legs = {"tanal": lambda: pv.tanal_device(x, w, starts, out), "compose": compose, "read_route": read_route}
            assert legs["tanal"]() == 0
            compose()
            torch.cuda.synchronize()
            same = bool(torch.equal(out.view(torch.int32), out_a.view(torch.int32)))
            t = interleaved(legs, args.reps)
            med = {k: float(np.median(v)) for k, v in t.items()}
            nbytes = x.numel() * 4 + out.numel() * 4
            print(json.dumps({"size": size, "hop": hop, "channels": C, "samples": samples, "factor": factor, "frames_out": Fout,
                              "bytes": nbytes, "bits_equal_compose": same,
                              "ms": {k: [round(u, 4) for u in v] for k, v in t.items()},
                              "gbs": {k: round(nbytes / med[k] / 1e6, 1) for k in legs},
                              "ratio": {"compose_over_tanal": round(med["compose"] / med["tanal"], 2),
                                        "read_route_over_tanal": round(med["read_route"] / med["tanal"], 2)},
                              "spread": {k: round((max(v) - min(v)) / med[k], 3) for k, v in t.items()},
                              "copy_gbs": round(copy_tbs * 1e3, 1), "kernel": pv.tanal_kernel_name()}), flush=True)
            del out, out_a, out_b, index, cspec, cfr, objs
            torch.cuda.empty_cache()
        del xpad, spec, grid
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
