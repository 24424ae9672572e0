"""coupling() on the host side (no GPU): the band-to-rows selector, the argument checks of gcwt_coupling before any
device call, the grid it launches (include/ghostcwt_debug.h: gcwt_debug_coupling_grid), and the float64 model of the
definition (tests/coupling_model.py) on the oracle's coefficients."""
import ctypes as C

import numpy as np
import pytest

import coupling_model as pm
from oracle import ghost_oracle as orc


# -- the selector -----------------------------------------------------------------------------------------------------
def test_rows_of_a_band_on_a_descending_grid():
    from ghost_amd.engine import coupling_rows
    f = 200.0 / 2 ** (np.arange(23) / 4.0)                  # 200 ... 4.42 Hz, the default grid's order
    assert coupling_rows((30, 200), f, "amplitude") == (0, 11)
    assert coupling_rows((4, 16), f, "phase") == (15, 8)
    assert coupling_rows((4.0, 1e9), f, "phase") == (0, 23)
    first, count = coupling_rows((7.0, 8.0), f, "phase")
    assert (first, count) == (19, 1) and 7.0 <= f[19] <= 8.0
    assert coupling_rows((np.float32(50), np.int64(100)), f, "amplitude") == (4, 5)


def test_rows_of_a_band_on_an_ascending_grid():
    from ghost_amd.engine import coupling_rows
    f = np.array([2.0, 4.0, 6.0, 8.0, 10.0, 40.0, 80.0])    # freqs=: sorted upwards
    assert coupling_rows((4, 8), f, "phase") == (1, 3)
    assert coupling_rows((30, 200), f, "amplitude") == (5, 2)
    assert coupling_rows([2, 80], f, "phase") == (0, 7)


def test_band_limits_are_inclusive_on_both_edges():
    from ghost_amd.engine import coupling_rows
    f = np.array([64.0, 32.0, 16.0, 8.0, 4.0])
    assert coupling_rows((8.0, 32.0), f, "phase") == (1, 3)
    assert coupling_rows((8.0, 8.0), f, "phase") == (3, 1)              # f_lo == f_hi on a row
    assert coupling_rows((np.nextafter(8.0, 9.0), 32.0), f, "phase") == (1, 2)
    assert coupling_rows((8.0, np.nextafter(32.0, 0.0)), f, "phase") == (2, 2)


@pytest.mark.parametrize("limits", [(9.0, 15.0), (100.0, 200.0), (0.1, 3.9), (16.0, 8.0), (8.0,), (4.0, 8.0, 16.0), 8.0, None,
                                    "48", ("4", "8"), (4.0, np.inf), (np.nan, 8.0), (True, 8.0), (4.0, None), (4 + 0j, 8.0)])
def test_selector_refuses_and_names_the_band(limits):
    from ghost_amd.engine import coupling_rows
    f = np.array([64.0, 32.0, 16.0, 8.0, 4.0])
    for what in ("phase", "amplitude"):
        with pytest.raises(ValueError, match=what):
            coupling_rows(limits, f, what)


def test_coupling_before_any_transform_raises():
    from ghost_amd.wave import ContinuousWaveletTransform
    with pytest.raises(ValueError, match="transform"):
        ContinuousWaveletTransform().coupling(phase=(4, 16), amplitude=(30, 200), window=64)
    with pytest.raises(ValueError, match="window"):
        ContinuousWaveletTransform().coupling(phase=(4, 16), amplitude=(30, 200), window=1)
    with pytest.raises(TypeError):
        ContinuousWaveletTransform().coupling(phase=(4, 16), amplitude=(30, 200))       # window is required
    with pytest.raises(TypeError):
        ContinuousWaveletTransform().coupling(amplitude=(30, 200), window=64)
    with pytest.raises(TypeError):
        ContinuousWaveletTransform().coupling((4, 16), (30, 200), window=64)            # keywords only


def test_engine_coupling_refuses_what_is_not_a_complex_device_result():
    from ghost_amd import engine
    from ghost_amd.multi import ShardedResult
    with pytest.raises(ValueError, match="one device"):
        engine.coupling(ShardedResult([], (4, 3, 100), True), (0, 1), (1, 2), 64)
    with pytest.raises(ValueError, match="complex"):
        engine.coupling(engine.DeviceResult(object(), (4, 3, 100), 128, False), (0, 1), (1, 2), 64)
    with pytest.raises(ValueError, match="window"):
        engine.coupling(engine.DeviceResult(object(), (4, 3, 100), 128, True), (0, 1), (1, 2), 1)
    for rows in ((0, 0), (-1, 2), (2, 2), (0, 4), (0.0, 1), (True, 1), (0,), None):
        with pytest.raises(ValueError, match="phase_rows"):
            engine.coupling(engine.DeviceResult(object(), (4, 3, 100), 128, True), rows, (1, 2), 64)
        with pytest.raises(ValueError, match="amp_rows"):
            engine.coupling(engine.DeviceResult(object(), (4, 3, 100), 128, True), (0, 3), rows, 64)


# -- the C entry point: arguments first, then the device ----------------------------------------------------------------
def test_entry_point_validates_then_needs_a_device():
    from ghost_amd import _lib
    from ghost_amd.engine import device_count
    lib = _lib.lib
    buf = (C.c_float * 64)()

    def call(rows=buf, pitch=16, c=1, s=4, n=16, p0=2, n_p=2, a0=0, n_a=3, window=4, vec=buf, mvl=buf, amp=buf, out_pitch=4):
        return lib.gcwt_coupling(rows, pitch, c, s, n, p0, n_p, a0, n_a, window, vec, mvl, amp, out_pitch)

    for kw, word in ((dict(rows=None), b"NULL"), (dict(window=1), b"window"), (dict(window=0), b"window"),
                     (dict(pitch=15), b"pitch"), (dict(n=0), b"n_cols"), (dict(s=0), b"n_scales"), (dict(c=0), b"n_channels"),
                     (dict(p0=-1), b"phase"), (dict(n_p=0), b"phase"), (dict(p0=3, n_p=2), b"phase"), (dict(p0=4, n_p=1), b"phase"),
                     (dict(a0=-1), b"amplitude"), (dict(n_a=0), b"amplitude"), (dict(n_a=5), b"amplitude"),
                     (dict(a0=2**31 - 1, n_a=2**31 - 1), b"amplitude"), (dict(out_pitch=3), b"out_pitch"),
                     (dict(vec=None, mvl=None, amp=None), b"nothing")):
        assert call(**kw) == _lib.ERR_INVALID, kw
        assert word in lib.gcwt_last_error(), (kw, lib.gcwt_last_error())
    # a valid request (the ranges overlap; two outputs left out): without a GPU there is nothing that computes it; with
    # one, host memory is not a resident result
    n_dev = device_count()
    for kw in (dict(), dict(p0=0, n_p=4, a0=0, n_a=4), dict(vec=None, amp=None)):
        rc = call(**kw)
        if n_dev == 0:
            assert rc == _lib.ERR_NO_DEVICE and b"no CPU path" in lib.gcwt_last_error()
        else:
            assert rc == _lib.ERR_INVALID and b"device memory" in lib.gcwt_last_error()


# -- the grid ------------------------------------------------------------------------------------------------------------
def _grid(c, n, n_p, n_a, window):
    from ghost_amd import _lib
    pt, at = C.c_int32(), C.c_int32()
    rb, nr, nb = C.c_int64(), C.c_int64(), C.c_int64()
    rc = _lib.lib.gcwt_debug_coupling_grid(c, n, n_p, n_a, window, C.byref(pt), C.byref(at), C.byref(rb), C.byref(nr), C.byref(nb))
    assert rc == 0, _lib.lib.gcwt_last_error()
    return pt.value, at.value, rb.value, nr.value, nb.value


def test_grid_covers_every_tile_of_every_channel_and_run():
    from ghost_amd import _lib
    for c, n, n_p, n_a, window in ((1, 5003, 1, 1, 2), (3, 5003, 5, 9, 100), (128, 1000000, 8, 11, 1000), (128, 1000000, 8, 11, 10000),
                                   (16, 1 << 18, 12, 20, 1000), (9, 5003, 4, 8, 5008), (2, 70000, 13, 17, 3)):
        pt, at, run_bins, n_runs, blocks = _grid(c, n, n_p, n_a, window)
        n_bins = -(-n // window)
        assert (pt, at) == (-(-n_p // 4), -(-n_a // 8))                          # tiles of 4 phase x 8 amplitude rows
        assert run_bins % 4 == 0 and run_bins >= 4                               # every wave of a workgroup has a bin
        assert (n_runs - 1) * run_bins < n_bins <= n_runs * run_bins             # the runs cover the bins, none is empty
        units = c * n_runs
        assert blocks == -(-units // 8) * 8 * pt * at and blocks < 2 ** 31       # tiles of a unit lie 8 workgroups apart
    assert _grid(128, 1000000, 8, 11, 1000)[:4] == (2, 2, 12, 84)
    # a grid that would not fit is cut into longer runs
    pt, at, run_bins, n_runs, blocks = _grid(30000, 1 << 31, 64, 64, 2)
    assert blocks < 2 ** 31 and run_bins > 4 * 1024
    assert _lib.lib.gcwt_debug_coupling_grid(1, 100, 1, 1, 1, None, None, None, None, None) == _lib.ERR_INVALID
    assert _lib.lib.gcwt_debug_coupling_grid(1, 100, 0, 1, 4, None, None, None, None, None) == _lib.ERR_INVALID
    assert _lib.lib.gcwt_debug_coupling_grid(1, 100, 1, 1, 4, None, None, None, None, None) == 0


# -- the model ---------------------------------------------------------------------------------------------------------------
def test_bounds_are_the_derived_ones():
    u = 2.0 ** -24
    assert pm.K == 6
    for w, chain in ((2, 1), (64, 1), (65, 2), (1000, 16), (5008, 79)):
        assert pm.vector_bound(w) == np.sqrt(2.0) * (6 + chain + 6 + 1) * u
        assert pm.amplitude_bound(w) == (2 + chain + 6 + 1) * u
        assert pm.mvl_bound(w) == pm.vector_bound(w) + pm.amplitude_bound(w) + 3 * u


def test_model_sums_are_the_definition():
    rng = np.random.default_rng(3)
    w = rng.standard_normal((2, 5, 23)) + 1j * rng.standard_normal((2, 5, 23))
    w[1, :, 10:20] = 0
    w[0, 1, 3] = 0                                                               # a phase sample without a direction
    m = pm.model(w, (1, 2), (2, 3), 5)
    assert m["vector"].shape == (2, 2, 3, 5) and m["mvl"].shape == (2, 2, 3, 5) and m["amplitude"].shape == (2, 3, 5)
    assert m["counts"].tolist() == [5, 5, 5, 5, 3]
    ph = np.angle(w[0, 2, 20:23])
    np.testing.assert_allclose(m["vector"][0, 1, 2, 4], np.mean(np.abs(w[0, 4, 20:23]) * np.exp(1j * ph)), rtol=1e-13)
    np.testing.assert_allclose(m["amplitude"][0, 0, 1], np.mean(np.abs(w[0, 2, 5:10])), rtol=1e-14)
    np.testing.assert_allclose(m["m"][0, 0, 1, 0], np.sum((np.abs(w[0, 3]) * np.exp(1j * np.angle(w[0, 1])))[[0, 1, 2, 4]]), rtol=1e-13)
    np.testing.assert_allclose(m["mvl"], np.abs(m["ratio"]), rtol=0, atol=0)
    assert np.all(m["mvl"][1, :, :, 2:4] == 0) and np.all(m["vector"][1, :, :, 2:4] == 0) and np.all(m["amplitude"][1, :, 2:4] == 0)
    assert m["mvl"].min() >= 0 and m["mvl"].max() <= 1 + 1e-12
    # a row against itself: all amplitude at every phase it has -- M = sum W, not 1; constant phase: exactly 1
    one = pm.model(np.abs(w[:1]) * np.exp(0.3j), (0, 1), (3, 1), 4)
    np.testing.assert_allclose(one["mvl"], 1.0, rtol=1e-12)
    np.testing.assert_allclose(np.angle(one["vector"]), 0.3, rtol=1e-12)
    same = pm.model(w[:1], (2, 1), (2, 1), 23)
    np.testing.assert_allclose(same["m"][0, 0, 0, 0], w[0, 2].sum(), rtol=1e-13)


def test_model_on_the_oracle_finds_the_coupled_channel_its_phase_and_the_uncoupled_one():
    from ghost_amd.engine import coupling_rows
    n, fs = 32768, 1000.0
    x = pm.coupled_input(n, fs)
    f = orc.frequency_grid(fs, n, freq_limits=(4, 200), voices_per_octave=4)
    ph, am = coupling_rows((4, 16), f, "phase"), coupling_rows((30, 200), f, "amplitude")
    assert ph[1] == 8 and am[1] == 11
    w = np.stack([orc.cwt_complex(x[c], fs, f) for c in range(2)])
    p8 = int(np.argmin(np.abs(f[ph[0]:ph[0] + ph[1]] - 8.0)))
    a80 = int(np.argmin(np.abs(f[am[0]:am[0] + am[1]] - 80.0)))
    for window in (1024, 4096):
        m = pm.model(w, ph, am, window)
        mvl0 = float(np.median(m["mvl"][0, p8, a80, 1:-1]))
        ang0 = float(np.median(np.angle(m["vector"][0, p8, a80, 1:-1])))
        mvl1 = float(np.median(m["mvl"][1, p8, a80, 1:-1]))
        gate = float(pm.gate_bound(w, ph, am, window).max())
        print("window %d: channel 0 mvl %.4f angle %.4f rad, channel 1 mvl %.4f; gate bound %.3g" % (window, mvl0, ang0, mvl1, gate))
        assert mvl0 >= 0.25
        assert abs(ang0 - 1.0) <= 0.03
        assert mvl1 <= 0.05
        assert gate <= 2e-3
