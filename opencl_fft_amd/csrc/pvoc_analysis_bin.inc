// pvoc_analysis_bin.inc — one bin of the Analysis of clfa_pvoc (include/clfft_amd.h), included inside the loop over the
// frames of k_pvoc_analyze (pvoc_kernels.hip) and over the bins of k_pvoc_tanal (tanal_kernels.hip): one copy of the
// expressions, so both give the same bits for the same pair of spectra.  A textual piece, not a function: inlining a
// function here reorders k_pvoc_analyze's instructions (profiles/pvoc_tanal_same.txt), and that kernel keeps the
// instructions it had.
// In scope: cpx z (this frame's bin), zp (the frame before), e (= e[k]); int k; float sh (size / hop), srs (sr / size).
// Defines: amp = |z|; d = z conj(zp) e; dev = atan2f(Im d, Re d) / (2 pi), 0 where d = (0, 0); freq = (k + dev sh) srs.
      const float amp = sqrtf(z.x * z.x + z.y * z.y);
      const float tx = z.x * zp.x + z.y * zp.y, ty = z.y * zp.x - z.x * zp.y;   // z conj(z_prev)
      const float dx = tx * e.x - ty * e.y, dy = tx * e.y + ty * e.x;
      const float dev = (dx == 0.f && dy == 0.f) ? 0.f : atan2f(dy, dx) * 0.15915494309189535f;   // turns
      const float freq = ((float)k + dev * sh) * srs;
