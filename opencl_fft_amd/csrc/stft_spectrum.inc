// stft_spectrum.inc — "windowed frames parked in LDS -> their packed spectra in LDS", included inside the loop over the
// groups of k_stft_analyze (stft_kernels.hip) and, twice per group, of k_pvoc_tanal (tanal_kernels.hip): one copy of the
// sequence, so both give the same bits for the same windowed frame.  A textual piece, as the kernel bodies of the FFT
// families are (fft_lds.inc): a function here changes k_stft_analyze's instructions, and that kernel keeps the ones it had.
// In scope: LOGN, G = LdsGeom<LOGN>, N, E, T; int t (the lane of its frame's T); cpx *xb (the frame's padded slot); s_tab
// and s_w2 (the twiddle and pair tables).  On entry the frames are parked and a barrier has passed; at the end the spectra
// are in the slots (element p at lds_pad(p)) and a barrier has passed.  Declares v.
    cpx v[E];
    pass_gather_padded<LOGN, G::LOGE>(v, t, xb);
    wg_passes<LOGN, G::LOGE, 0, true>(v, t, s_tab, xb);
#pragma unroll
    for (int e = 0; e < E; e++) v[e] = cscale(v[e], 1.0f / (float)N);   // forward real plans scale by 1/M (cl_fft.cpp:39)
    __syncthreads();
    dif_scatter_padded<LOGN, G::LOGE>(v, t, xb);
    __syncthreads();
    // reference `conv` (cl_fft.cpp:178-191) on the natural-order copy; pair 0 = packed DC / Nyquist, bin N/2 untouched
#pragma unroll
    for (int k = 0; k < E / 2; k++) {
      const int i = t + T * k, j = i == 0 ? N / 2 : N - i;
      const cpx ci = xb[lds_pad(i)], cj = xb[lds_pad(j)];
      cpx oi, oj;
      r2c_pair(ci, cj, s_w2[i], oi, oj);
      const bool z = i == 0;
      oi = mk(z ? (ci.x + ci.y) * .5f : oi.x, z ? (ci.x - ci.y) * .5f : oi.y);
      oj = mk(z ? cj.x : oj.x, z ? cj.y : oj.y);
      xb[lds_pad(i)] = oi;
      xb[lds_pad(j)] = oj;
    }
    __syncthreads();
