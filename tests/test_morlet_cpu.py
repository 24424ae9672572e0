"""Morlet wavelets through transform(): the Python surface, the closed-form response and host-only planning
(CPU only, no compute calls)."""
import ctypes as C

import numpy as np
import pytest

import morlet_model
from ghost_amd import _lib
from ghost_amd._lib import GhostCwtError
from ghost_amd.engine import CwtPlan
from ghost_amd.wave import Morlet

CASES = [(6.0, 1000.0), (5.0, 1250.0), (10.0, 30000.0)]
BAND_TOL = 2e-7                  # gcwt_params.band_eps' default (ghostcwt.h)


def _default_grid(m, n, fs, voices=10):
    """transform()'s grid arithmetic (wave/transforms.py: freq_bounds_ref, n_octaves, j)."""
    lo, hi = np.array(m.compute_freq_bounds(n)) / np.pi * fs / 2.0
    n_octaves = np.log2(hi / lo)
    j = np.arange(np.floor(n_octaves * voices) + 1)
    return hi / 2 ** (j / voices)


def test_lengths_equal_the_kernels(golden):
    g = golden("G16_morlet.npz")
    for w0, fs in CASES:
        tag = "%g_%g" % (w0, fs)
        m = Morlet(w0=w0, fs=fs)
        freqs = g["frequencies_" + tag]
        lengths = m.compute_lengths(freqs / (fs / 2.0) * np.pi)
        np.testing.assert_array_equal(lengths, g["lengths_" + tag])
        np.testing.assert_array_equal(lengths, [len(g["psi_%s_%d" % (tag, k)]) for k in range(len(freqs))])
        # this repository's class makes the reference's numbers
        for k in (0, len(freqs) - 1):
            np.testing.assert_allclose(Morlet(w0=w0, freq=freqs[k], fs=fs).get_wavelet(), g["psi_%s_%d" % (tag, k)],
                                       rtol=0, atol=1e-12)     # (golden G10 pins it to the ulp)


def test_lengths_over_a_sweep_and_near_integers():
    for w0, fs in CASES:
        m = Morlet(w0=w0, fs=fs)
        lo, hi = np.array(m.compute_freq_bounds(100000)) / np.pi * fs / 2.0
        freqs = list(np.geomspace(lo, hi, 200))
        # frequencies where M + 1 = 15 sigma + 1 is within 1e-9 of an integer, from either side
        kappa = (w0 + np.sqrt(2 + w0 ** 2)) / 2
        for target in (50, 333, 4096, 19999):
            for eps in (-1e-9, -1e-12, 0.0, 1e-12, 1e-9):
                sigma = (target - 1 + eps) / 15.0
                freqs.append(kappa / sigma / (2 * np.pi) * fs)
        freqs = np.array(freqs)
        lengths = m.compute_lengths(freqs / (fs / 2.0) * np.pi)
        hz = freqs / (fs / 2.0) * np.pi / np.pi * fs / 2.0          # the Hz transform() hands the library
        real = [len(Morlet(w0=w0, freq=f, fs=fs).get_wavelet()) for f in hz]
        np.testing.assert_array_equal(lengths, real)


def test_freq_bounds_closed_forms():
    for w0 in (5.0, 6.0, 10.0):
        m = Morlet(w0=w0)
        kappa = (w0 + np.sqrt(2 + w0 ** 2)) / 2
        for n in (4096, 100000, 1000000):
            lo, hi = m.compute_freq_bounds(n)
            assert lo == pytest.approx(kappa / ((n // 5 - 1) / 15.0), rel=1e-14)
            assert hi == pytest.approx(kappa * np.pi / (w0 + np.sqrt(2 * np.log(10.0))), rel=1e-14)
        lo7, hi2 = m.compute_freq_bounds(100000, p=7, eta=0.2)
        assert lo7 == pytest.approx(kappa / ((100000 // 7 - 1) / 15.0), rel=1e-14)
        assert hi2 == pytest.approx(kappa * np.pi / (w0 + np.sqrt(2 * np.log(5.0))), rel=1e-14)
    m = Morlet(w0=6)
    for bad in (0, -6):                          # the class's own setter refuses them
        with pytest.raises(ValueError):
            m.w0 = bad


def test_default_grid_1e6_at_1khz():
    n, fs = 1000000, 1000.0
    m = Morlet(w0=6, fs=fs)
    lo, hi = np.array(m.compute_freq_bounds(n)) / np.pi * fs / 2.0
    assert lo == pytest.approx(0.0726, abs=5e-5) and hi == pytest.approx(373.33, abs=5e-3)
    f = _default_grid(m, n, fs)
    assert f.size == 124
    assert f[0] == pytest.approx(373.33, abs=5e-3) and f[-1] == pytest.approx(0.0740, abs=5e-5)
    lengths = m.compute_lengths(f / (fs / 2.0) * np.pi)
    assert lengths.max() <= n // 5
    # the top scale: 40 taps, and the literal kernel answers at Nyquist with 0.1 of its peak (the bound is set on the
    # un-aliased Gaussian, so not exactly)
    psi = Morlet(w0=6, freq=f[0], fs=fs).get_wavelet()
    assert len(psi) == 40 == lengths[0]
    theta = np.linspace(0, np.pi, 20001)
    h = np.abs(morlet_model.dtft(psi, theta))
    assert h[-1] / h.max() == pytest.approx(0.1, abs=1e-6)


def test_closed_form_against_the_golden_kernels(golden):
    g = golden("G16_morlet.npz")
    theta = np.linspace(-np.pi, np.pi, 2001)
    worst = 0.0
    for w0, fs in CASES:
        tag = "%g_%g" % (w0, fs)
        for k, f in enumerate(g["frequencies_" + tag]):
            psi = g["psi_%s_%d" % (tag, k)]
            ref = morlet_model.dtft(psi, theta)
            got = morlet_model.response(theta, w0, f, fs)
            err = np.abs(got - ref).max() / np.abs(ref).max()
            worst = max(worst, err)
            assert err <= 1e-10, (w0, fs, f, err)
    print("closed form against the DTFT of the golden kernels: worst %.2e of the peak" % worst)


def _plan(n, fs, freqs, **kw):
    return CwtPlan(n, 1, fs, freqs, **kw)


def _raw_create(flags, gamma=6.0, beta=0.0, reserved0=0):
    """gcwt_plan_create with the fields set by hand: the status."""
    freqs = np.array([40.0, 10.0])
    bounds = np.array([[0, 4096]], dtype=np.int64)
    p = _lib.Params()
    p.n_samples, p.n_channels, p.n_freqs = 4096, 1, 2
    p.fs, p.gamma, p.beta = 1000.0, gamma, beta
    p.freqs_hz = freqs.ctypes.data_as(C.POINTER(C.c_double))
    p.n_epochs = 1
    p.epoch_bounds = bounds.ctypes.data_as(C.POINTER(C.c_int64))
    p.device = -1
    p.wavelet_flags = flags
    p.reserved0 = reserved0
    h = C.c_void_p()
    rc = _lib.lib.gcwt_plan_create(C.byref(h), C.byref(p))
    if rc == 0:
        _lib.lib.gcwt_plan_destroy(h)
    return rc


def test_morlet_flag_on_the_c_abi():
    assert _lib.lib.gcwt_abi_version() == 5
    assert _lib.WAVELET_MORLET == 0x200
    assert _raw_create(_lib.WAVELET_MORLET) == 0                        # beta is ignored
    assert _raw_create(_lib.WAVELET_MORLET, beta=20.0) == 0
    assert _raw_create(_lib.WAVELET_MORLET | 1) == _lib.ERR_INVALID     # order bits
    assert _raw_create(_lib.WAVELET_MORLET | _lib.WAVELET_ENERGY) == _lib.ERR_INVALID
    assert _raw_create(_lib.WAVELET_MORLET, gamma=0.0) == _lib.ERR_INVALID
    assert _raw_create(_lib.WAVELET_MORLET, reserved0=7) == _lib.ERR_INVALID
    assert _raw_create(0, gamma=3.0, beta=20.0, reserved0=7) == _lib.ERR_INVALID
    assert _raw_create(0, gamma=3.0, beta=0.0) == _lib.ERR_INVALID      # a Morse plan still needs beta
    with pytest.raises(ValueError):
        CwtPlan(4096, 1, 1000.0, [40.0], morlet_w0=6.0, order=1)
    with pytest.raises(ValueError):
        CwtPlan(4096, 1, 1000.0, [40.0], morlet_w0=6.0, normalization="energy")


def test_planned_lengths_equal_the_python_ones():
    for w0, fs in CASES:
        m = Morlet(w0=w0, fs=fs)
        f = _default_grid(m, 200000, fs)
        with _closing(_plan(200000, fs, f, morlet_w0=w0)) as p:
            si = p.scale_info()
        np.testing.assert_array_equal(si["length"], m.compute_lengths(f / (fs / 2.0) * np.pi))


def test_band_limited_scales_take_the_fast_path():
    """N = 1e6, fs = 1 kHz, w0 = 6: every scale whose response is below band_tol of its peak outside a band no wider
    than pi -- on the float64 model, theta_hi + theta_neg <= pi -- can be decimated by two at least, so it must be
    planned GCWT_SCALE_SPECTRAL with decimation >= 2: the fast path is really used."""
    n, fs, w0 = 1000000, 1000.0, 6.0
    m = Morlet(w0=w0, fs=fs)
    f = _default_grid(m, n, fs)
    xi_hi, xi_neg = morlet_model.band(w0, BAND_TOL)
    sigma = np.array([morlet_model.geometry(w0, fk, fs)[0] for fk in f])
    limited = (xi_hi + xi_neg) / sigma <= np.pi
    assert limited.sum() >= 110                                          # all but the top octave or so
    with _closing(_plan(n, fs, f, morlet_w0=w0)) as p:
        si = p.scale_info()
        info = p.info
    assert np.all(si["method"][limited] == _lib.SCALE_SPECTRAL)
    assert np.all(si["decimation"][limited] >= 2)
    assert info["n_interp"] == 0
    assert si["decimation"].max() >= 16                                  # levels with R >= 16 exist


class _closing:
    def __init__(self, plan):
        self.plan = plan

    def __enter__(self):
        return self.plan

    def __exit__(self, *exc):
        self.plan.close()


def test_w0_below_five_is_planned_as_asked():
    m = Morlet(w0=4.0, fs=1000.0)
    f = _default_grid(m, 100000, 1000.0)
    with _closing(_plan(100000, 1000.0, f, morlet_w0=4.0)) as p:
        si = p.scale_info()
    np.testing.assert_array_equal(si["length"], m.compute_lengths(f / 500.0 * np.pi))
    assert GhostCwtError is not None
