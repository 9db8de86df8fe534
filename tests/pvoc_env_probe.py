"""Probe frames for the cepstral envelope of clfa_pvoc (pvoc_env.hpp: k_pvoc_formant, k_pvoc_vocode), numpy only.

Frames are (C, F, M + 1, 2) float32, M = size / 2; b = c F + f is the flat frame index, which is what the kernels group
by: a workgroup takes FPW consecutive frames b, whatever channel they belong to.

  even b  an impulse frame: every amp 1 except bin k0, which is A.  k0 runs through K0 of the size (the ends, the bins
          around the lane count T of the pair loop i = t + T k, around 16, around M / 2 and below M), then comes from a
          seeded generator; A cycles 256, 1 / 256, 0 (the 0 takes the floor 1e-20: |log| = 46).
  odd b   a constant frame: every amp 2^40 and 2^-40 alternately.  Its envelope is the constant itself, so a slot of a
          group leaking into its neighbour changes either kind of frame grossly.
  freq    any finite value; every operation on these frames must hand it back as copied bits.
"""
import numpy as np

f32 = np.float32
SIZES = (64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384)
AMPS = (f32(256), f32(1 / 256), f32(0))
HI, LO = f32(2.0 ** 40), f32(2.0 ** -40)


def lanes(size):
    """T of LdsGeom: lanes per transform, 16 points each"""
    return max(size // 2 // 16, 1)


def fpw(size):
    """frames per workgroup: at least 256 lanes"""
    t = lanes(size)
    return max(t, 256) // t


def k0_list(size):
    M, T = size // 2, lanes(size)
    out = []
    for k in [0, 1, 2, 3, T - 1, T, T + 1, 15, 16, 17, M // 2 - 1, M // 2, M // 2 + 1, M - 3, M - 2, M - 1, M]:
        k = min(max(k, 0), M)
        if k not in out:
            out.append(k)
    return out


def coefs_for(size):
    M, T = size // 2, lanes(size)
    out = []
    for c in [1, 2, T - 1, T, T + 1, M // 2 - 1, M // 2, M // 2 + 1, M - 2, M - 1]:
        c = min(max(c, 1), M - 1)
        if c not in out:
            out.append(c)
    return out


def channels_for(size):
    """2: the groups straddle the channel boundary wherever FPW > 1.  With FPW = 2 (size 4096) an even number of frames
    never leaves a ragged group, so that size takes 3 channels of an odd F: its boundaries fall inside groups too."""
    return 3 if fpw(size) == 2 else 2


def frames_for(size, C):
    """the smallest F >= 40 for which C F is at least three full groups of FPW frames plus a ragged remainder (FPW = 1: no
    group is ragged)"""
    w = fpw(size)
    for F in range(40, 40 + 4 * w + 2):
        n = C * F
        if w == 1 or (n > 3 * w and n % w != 0):
            return F
    raise ValueError("no ragged frame count for size %d with %d channels" % (size, C))


def impulses(size, count):
    """(k0, A) of the first `count` impulse frames"""
    M = size // 2
    ks = k0_list(size)
    rng = np.random.default_rng(size)
    more = rng.integers(0, M + 1, max(count - len(ks), 0)).tolist()
    return [((ks + more)[i], AMPS[i % 3]) for i in range(count)]


_PROBES = {}


def probe(size, C, F):
    key = (size, C, F)
    if key not in _PROBES:
        M = size // 2
        n = C * F
        fr = np.empty((n, M + 1, 2), f32)
        fr[..., 1] = np.random.default_rng(size + 1).uniform(-24000.0, 24000.0, (n, M + 1)).astype(f32)
        fr[0::2, :, 0] = 1
        for i, (k0, A) in enumerate(impulses(size, (n + 1) // 2)):
            fr[2 * i, k0, 0] = A
        odd = np.arange(1, n, 2)
        fr[odd, :, 0] = np.where((odd // 2) % 2 == 0, HI, LO)[:, None]
        fr = fr.reshape(C, F, M + 1, 2)
        fr.setflags(write=False)
        _PROBES[key] = fr
    return _PROBES[key]


def probe_for(size):
    C = channels_for(size)
    return probe(size, C, frames_for(size, C))
