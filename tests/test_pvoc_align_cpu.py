"""The alignment rule of clfa_pvoc's device forms (include/clfft_amd.h), for every form and every pointer it looks at:
frames, spectra and pairs on 8 bytes, float arrays on 4.  It is an argument check, so it answers before any device
lookup and this test runs without a GPU.  The blocking forms copy their arrays and take any address; an array an op
does not look at may lie anywhere."""
import numpy as np

import opencl_fft_amd as fa
from opencl_fft_amd import _lib

CL_INVALID_VALUE = -30
CL_INVALID_OPERATION = -59
SR = 48000.0
f32 = np.float32
SIZE, HOP, C, F, COEFS = 64, 16, 2, 3, 10
M = SIZE // 2


class _Buf:
    """the bytes of an array with room to lie a few bytes past an 8-byte boundary: on the device where there is one (the
    device forms launch on what they accept), else on the host"""

    def __init__(self, a, device):
        self.a = np.ascontiguousarray(a).view(np.uint8).ravel()
        if device:
            import torch
            self.mem = torch.zeros(self.a.size + 16, dtype=torch.uint8, device="cuda:0")
            self.base = self.mem.data_ptr()
        else:
            self.mem = np.zeros(self.a.size + 16, np.uint8)
            self.base = self.mem.ctypes.data
        self.first = -self.base % 8

    def at(self, off=0):
        """the address `off` bytes past the boundary, the array's values there"""
        s = self.first + off
        if isinstance(self.mem, np.ndarray):
            self.mem[s:s + self.a.size] = self.a
        else:
            import torch
            self.mem[s:s + self.a.size] = torch.from_numpy(self.a)
        assert (self.base + s) % 8 == off
        return self.base + s


def _cases():
    """(name, dev symbol, blocking symbol, {argument: (array, alignment, looked at)}, arguments of the call from the
    addresses), for every device form and op; the values are ones the blocking forms accept"""
    rng = np.random.default_rng(8)
    B = M + 1
    fr = np.stack([np.abs(rng.standard_normal((C, F, B))).astype(f32) + f32(0.01),
                   np.broadcast_to(np.arange(B) * (SR / SIZE), (C, F, B)).astype(f32)], axis=-1)
    spec = (rng.standard_normal((C, F, M)) + 1j * rng.standard_normal((C, F, M))).astype(np.complex64)
    half, one = np.full(F, 0.5, f32), np.ones(F, f32)
    table = np.linspace(0, 1, B).astype(f32)
    rows = {0: (100.0, 200.0, 3000.0, 4000.0), 1: (0.5,), 2: (0.5, 1.0), 3: (0.3, 0.9, 2.0), 4: (1.0, 0.01), 5: (1.5, 100.0, 1.0)}
    out = np.zeros_like(fr)
    cases = [
        ("analyze", "clfa_pvoc_analyze_dev", "clfa_pvoc_analyze", {"spectra": (spec, 8, True), "frames": (out, 8, True)},
         lambda p: (p["spectra"], p["frames"], F)),
        ("synthesize", "clfa_pvoc_synthesize_dev", "clfa_pvoc_synthesize",
         {"frames": (fr, 8, True), "spectra": (np.zeros_like(spec), 8, True)}, lambda p: (p["frames"], p["spectra"], F)),
        ("scale", "clfa_pvoc_scale_dev", "clfa_pvoc_scale", {"in": (fr, 8, True), "out": (out, 8, True), "par": (one, 4, True)},
         lambda p: (p["in"], p["out"], F, p["par"], 1, 1.0, COEFS)),
        ("shift", "clfa_pvoc_shift_dev", "clfa_pvoc_shift", {"in": (fr, 8, True), "out": (out, 8, True), "par": (one, 4, True)},
         lambda p: (p["in"], p["out"], F, p["par"], 1, 1, 1.0, COEFS)),
        ("read", "clfa_pvoc_read_dev", "clfa_pvoc_read", {"in": (fr, 8, True), "pos": (one, 4, True), "out": (out, 8, True)},
         lambda p: (p["in"], F, p["pos"], p["out"], F)),
        ("desc", "clfa_pvoc_desc_dev", "clfa_pvoc_desc", {"in": (fr, 8, True), "desc": (np.zeros((C, F, 8), f32), 4, True)},
         lambda p: (p["in"], p["desc"], F, 0, B, 0)),
    ]
    for op, name in enumerate(("cross", "morph", "filter", "mix", "vocode")):
        cases.append((name, "clfa_pvoc_pair_dev", "clfa_pvoc_pair",
                      {"a": (fr, 8, True), "b": (fr[::-1], 8, True), "out": (out, 8, True), "p": (half, 4, name != "mix"),
                       "q": (half, 4, name != "mix")},
                      lambda p, op=op: (op, p["a"], p["b"], p["out"], F, p["p"], p["q"], COEFS)))
    for op, name in enumerate(("band", "mask", "stencil", "arp", "lock", "warp")):
        par = np.zeros((F, 4), f32)
        par[:, :len(rows[op])] = rows[op]
        cases.append((name, "clfa_pvoc_shape_dev", "clfa_pvoc_shape",
                      {"in": (fr, 8, True), "out": (out, 8, True), "par": (par, 4, True),
                       "table": (table, 4, name in ("mask", "stencil"))},
                      lambda p, op=op: (op, p["in"], p["out"], F, p["par"], p["table"], 0, 1, COEFS)))
    for op, name in enumerate(("blur", "smooth", "freeze")):
        cases.append((name, "clfa_pvoc_time_dev", "clfa_pvoc_time",
                      {"in": (fr, 8, True), "out": (out, 8, True), "p": (one, 4, True), "q": (half, 4, name != "blur")},
                      lambda p, op=op: (op, p["in"], p["out"], F, p["p"], p["q"])))
    sig = np.zeros((C, F * HOP), f32)
    for fmod in (True, False):
        cases.append(("adsyn" + ("+fmod" if fmod else ""), "clfa_pvoc_adsyn_dev", "clfa_pvoc_adsyn",
                      {"frames": (fr, 8, True), "fmod": (one, 4, True), "signal": (sig, 4, True)} if fmod else
                      {"frames": (fr, 8, True), "signal": (sig, 4, True)},
                      lambda p: (p["frames"], F, p.get("fmod"), 0, B, 1, 1.0, p["signal"], F * HOP)))
    return cases


def test_device_forms_refuse_a_misaligned_pointer_and_blocking_forms_take_it():
    pv = fa.Pvoc(0, SIZE, HOP, SR, C)
    good = pv.get_error()                  # 0 with a device, "Device not found" without: what a good call returns
    assert good == (0 if fa.device_count() > 0 else -1)
    assert pv.blur_setup(4) == good
    L = _lib.lib()
    seen = 0
    for name, dev, blocking, arrays, args in _cases():
        host = {k: _Buf(a, False) for k, (a, _, _) in arrays.items()}
        there = {k: _Buf(a, good == 0) for k, (a, _, _) in arrays.items()}
        off = {k: 4 if align == 8 else 2 for k, (_, align, _) in arrays.items()}

        def devf(bad=None):
            return getattr(L, dev)(pv._h, *args({k: b.at(off[k] if k == bad else 0) for k, b in there.items()}), None)

        def hostf(bad=None):
            return getattr(L, blocking)(pv._h, *args({k: b.at(off[k] if k == bad else 0) for k, b in host.items()}))

        # a good call: the blur cannot be set up without a device, and says so before the object's error
        want = CL_INVALID_OPERATION if name == "blur" and good != 0 else good
        assert hostf() == want, name
        # analysis and synthesis report the object's own error ahead of their arrays, the other forms behind them
        refused = good if good != 0 and name in ("analyze", "synthesize") else CL_INVALID_VALUE
        for k, (_, _, looked_at) in arrays.items():
            assert hostf(k) == want, (name, k)
            assert devf(k) == (refused if looked_at else want), (name, k)
            seen += 1
        assert devf() == want, name        # on device memory where there is a device: the addresses alone were not it
    assert seen == 2 * 2 + 3 * 3 + 2 + 5 * 5 + 6 * 4 + 3 * 4 + 3 + 2
    if good == 0:
        import torch
        torch.cuda.synchronize()
