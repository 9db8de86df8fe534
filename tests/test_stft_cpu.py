"""Short-time transforms (clfa_stft) without a GPU: argument checks before any device lookup, the frame / length
formulas, the packed <-> one-sided layout map, and the float64 overlap-add model the GPU tests measure against."""
import numpy as np
import pytest

import opencl_fft_amd as fa
from oracle import oracle
from tests import stft_model

CL_INVALID_VALUE = -30
CL_DEVICE_NOT_FOUND = -1


@pytest.mark.parametrize("size,hop", [(1000, 4), (32, 8), (32768, 8), (0, 1), (-64, 1), (96, 4), (1024, 0), (1024, -1),
                                      (1024, 1025)])
def test_invalid_arguments_without_a_device(size, hop):
    st = fa.Stft(0, size, hop)
    assert st.get_error() == CL_INVALID_VALUE, st.get_log()


@pytest.mark.parametrize("size,hop", [(64, 1), (64, 64), (2048, 512), (16384, 3), (16384, 16384)])
def test_valid_arguments_reach_the_device_lookup(size, hop):
    if fa.device_count() > 0:
        pytest.skip("a device is present: creation succeeds (tests/test_gpu_stft.py)")
    st = fa.Stft(0, size, hop, window=np.hanning(size).astype(np.float32))
    assert st.get_error() == CL_DEVICE_NOT_FOUND


def test_window_length_checked():
    with pytest.raises(ValueError):
        fa.Stft(0, 256, 64, window=np.ones(255, np.float32))


@pytest.mark.parametrize("size,hop", [(64, 1), (64, 3), (256, 64), (2048, 512), (1024, 1024)])
def test_frame_and_sample_formulas(size, hop):
    st = fa.Stft(0, size, hop)
    for samples in (0, 1, size - 1, size, size + 1, size + hop - 1, size + hop, 5 * size + 7, 123457):
        want = 0 if samples < size else 1 + (samples - size) // hop
        assert st.frames(samples) == want == stft_model.frames_of(size, hop, samples)
    assert st.samples(0) == 0
    for F in (1, 2, 17, 1000):
        assert st.samples(F) == (F - 1) * hop + size
        assert st.frames(st.samples(F)) == F


@pytest.mark.parametrize("size", [64, 256, 2048, 16384])
def test_packed_to_onesided_matches_numpy_rfft(size):
    x = np.random.default_rng(size).standard_normal((5, size)).astype(np.float32)
    P = oracle.rfft_forward(x)                       # the library's packed layout and scaling (Clrfft forward)
    X = fa.packed_to_onesided(P.astype(np.complex128))
    R = np.fft.rfft(x.astype(np.float64), axis=-1)
    assert X.shape == R.shape == (5, size // 2 + 1)
    err = np.abs(X - R).max(axis=-1) / np.abs(R).max(axis=-1)
    assert err.max() <= 1e-6, err
    M = size // 2
    e_mid = np.abs(X[:, M // 2] - R[:, M // 2]).max() / np.abs(R).max()   # bin M/2: the reference's unconjugated bin
    assert e_mid <= 1e-6
    back = fa.onesided_to_packed(R)
    assert np.abs(back - P).max() / np.abs(P).max() <= 1e-6


def test_layout_map_torch_and_numpy_agree():
    torch = pytest.importorskip("torch")
    P = oracle.rfft_forward(np.random.default_rng(3).standard_normal((2, 7, 128)).astype(np.float32))
    Xn = fa.packed_to_onesided(P)
    Xt = fa.packed_to_onesided(torch.from_numpy(P))
    assert np.allclose(Xt.numpy(), Xn, rtol=1e-6, atol=1e-6)
    assert np.allclose(fa.onesided_to_packed(Xt).numpy(), fa.onesided_to_packed(Xn), rtol=1e-6, atol=1e-6)


def test_overlap_add_model_by_hand():
    # size 4, hop 2, two frames: y = [w0 r00, w1 r01, w2 r02 + w0 r10, w3 r03 + w1 r11, w2 r12, w3 r13]
    w = np.array([1.0, 2.0, 3.0, 4.0])
    r = np.array([[[1.0, 1.0, 1.0, 1.0], [10.0, 20.0, 30.0, 40.0]]])
    y, env = stft_model.overlap_add(r, w, 2)
    assert np.array_equal(y[0], [1, 2, 3 + 10, 4 + 40, 90, 160])
    assert np.array_equal(env, [1, 4, 9 + 1, 16 + 4, 9, 16])
    yn, _ = stft_model.overlap_add(r, w, 2, normalize=True)
    assert np.allclose(yn[0], np.array([1, 2, 13, 44, 90, 160]) / env)
    # a zero window sample leaves the output as it is there
    w0 = np.array([0.0, 1.0, 1.0, 0.0])
    y0, env0 = stft_model.overlap_add(np.ones((1, 1, 4)), w0, 4, normalize=True)
    assert env0[0] == 0 and y0[0, 0] == 0 and y0[0, 1] == 1


def test_frame_view_is_the_definition():
    x = np.arange(2 * 23, dtype=np.float32).reshape(2, 23)
    v = stft_model.frame_view(x, 8, 5)
    assert v.shape == (2, 4, 8)
    for c in range(2):
        for f in range(4):
            assert np.array_equal(v[c, f], x[c, f * 5:f * 5 + 8])
