"""The index arithmetic of the overlap-add synthesis (opencl_fft_amd/csrc/stft_plan.hpp) on the CPU, exhaustively: the
window envelope's lookup against a direct float64 sum for every (size, hop, F, sample) of three small sizes, and the split
of a channel into runs for every frame count up to 3000 at the shapes tests/test_gpu_stft_synth.py runs on the device."""
import os
import subprocess

from tests import stft_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "stft_plan.hpp"

#include <cmath>
#include <cstdio>
#include <vector>

using namespace clfa;

static const int kPairs[][2] = {@PAIRS@};

int main() {
  long bad = 0;
  // ---- envelope: every hop, every F up to 2 ceil(size / hop) + 2, every sample, three windows -----------------------
  long hits[4] = {0, 0, 0, 0}, zeros = 0, checked = 0;
  double worst = 0;
  const double bound = std::ldexp(1.0, -24) * (1 + 1e-6);
  const double pi = std::acos(-1.0);
  for (int size : {8, 16, 64}) {
    for (int kind = 0; kind < 3; kind++) {
      std::vector<float> w(size);
      for (int d = 0; d < size; d++) {
        if (kind == 0) w[d] = (float)(1 + ((d * 40503) >> 4) % 31);                 // integers
        else w[d] = (float)(0.5 - 0.5 * std::cos(2 * pi * d / size));               // periodic hann
        if (kind == 2 && d >= size / 4 && d < size / 4 + size / 2) w[d] = 0.f;      // ... with a stretch of zeros
      }
      for (int hop = 1; hop <= size; hop++) {
        std::vector<double> cum(2 * (size_t)size);
        stft_env_table(w.data(), size, hop, cum.data());   // the table stft_setup uploads
        const int fmax = 2 * ((size + hop - 1) / hop) + 2;
        for (int F = 1; F <= fmax; F++) {
          const long L = (long)(F - 1) * hop + size;
          for (long p = 0; p < L; p++) {
            double want = 0;
            for (int f = 0; f < F; f++) {
              const long d = p - (long)f * hop;
              if (d >= 0 && d < size) want += (double)w[d] * w[d];
            }
            int dl, dh;
            hits[stft_env_span(size, hop, F, p, dl, dh)]++;
            const double got = stft_env_at(cum.data(), size, hop, F, p);
            checked++;
            bool ok;
            if (want == 0) {
              zeros++;
              ok = got == 0;
            } else {
              const double rel = std::fabs(got - want) / want;
              worst = rel > worst ? rel : worst;
              ok = rel <= bound;
            }
            if (!ok && bad++ < 10)
              printf("env: window %d size %d hop %d F %d p %ld: got %.17g want %.17g\n", kind, size, hop, F, p, got, want);
          }
        }
      }
    }
  }
  printf("envelope: %ld samples, branch hits %ld / %ld / %ld, exact zeros %ld, worst relative error %.3g (bound %.3g)\n",
         checked, hits[1], hits[2], hits[3], zeros, worst, bound);
  const bool covered = hits[1] >= 1000 && hits[2] >= 1000 && hits[3] >= 1000 && zeros >= 1000;

  // ---- runs: every F up to 3000, every nf the launcher can produce --------------------------------------------------
  long splits = 0, multi = 0;
  for (const auto &pr : kPairs) {
    const int size = pr[0], hop = pr[1], fpw = stft_fpw(size);
    const int warm = (size + hop - 1) / hop;
    const long floor_nf = 8L * warm > fpw ? 8L * warm : fpw;
    for (int F = 1; F <= 3000; F++) {
      const int nf_min = (int)(floor_nf < F ? floor_nf : F);
      // the launcher's nf lies in [nf_min, F] whatever the device and the channel count
      for (long slots : {1L, 7L, 256L, 512L, 2048L})
        for (long ch : {1L, 3L, 200L}) {
          const int nf = stft_run_frames(ch * F, slots, size, hop, fpw, F);
          if ((nf < nf_min || nf > F) && bad++ < 10) printf("nf: size %d hop %d F %d slots %ld ch %ld: %d\n", size, hop, F, slots, ch, nf);
        }
      const long L = (long)(F - 1) * hop + size;
      for (int nf = nf_min; nf <= F; nf++) {
        const int runs = stft_runs(F, nf);
        long at = 0;   // the samples below `at` are owned by the runs before r
        bool ok = runs >= 1 && (long)(runs - 1) * nf < F && (long)runs * nf >= F;
        for (int r = 0; r < runs && ok; r++) {
          const StftRun u = stft_run(r, nf, F, size, hop);
          const long hi = r == runs - 1 ? L : (long)u.e_end * hop;
          ok = ok && u.s == r * nf && u.e_end > u.s && u.e_end <= F && (r == runs - 1) == (u.e_end == F);
          ok = ok && u.own_lo == (long)u.s * hop && u.own_lo == at && hi > at;
          // fw: the smallest frame with fw hop + size > own_lo, and never after the run's first frame
          ok = ok && u.fw >= 0 && (long)u.fw * hop + size > u.own_lo && (u.fw == 0 || (long)(u.fw - 1) * hop + size <= u.own_lo);
          ok = ok && u.fw <= u.s;
          at = hi;
        }
        ok = ok && at == L;
        splits++;
        multi += runs > 1;
        if (!ok && bad++ < 10) printf("runs: size %d hop %d F %d nf %d runs %d\n", size, hop, F, nf, runs);
      }
    }
  }
  printf("runs: %ld splits checked, %ld with more than one run\n", splits, multi);
  const bool all = bad == 0 && covered && multi > 1000;
  printf(all ? "OK\n" : "FAIL (%ld mismatches)\n", bad);
  return all ? 0 : 1;
}
"""


def test_envelope_lookup_and_run_split_exhaustively(tmp_path):
    """stft_env_at within one float32 rounding of the float64 direct sum (exactly 0 where that is 0), each of its three
    forms taken at least 1000 times; the runs' owned ranges tile [0, L), fw is the first frame that reaches own_lo"""
    pairs = ", ".join("{%d, %d}" % p for p in stft_model.SYNTH_PAIRS)
    src, exe = tmp_path / "stft_plan_check.cpp", str(tmp_path / "stft_plan_check")
    src.write_text(PROGRAM.replace("@PAIRS@", pairs))
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "opencl_fft_amd", "csrc"), str(src),
                           "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = p.stdout.decode()
    print(out)
    assert p.returncode == 0 and out.strip().endswith("OK"), out
