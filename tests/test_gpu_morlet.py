"""Morlet wavelets through transform() on the MI355X.  Row f of every result is the 'same'-mode convolution of the
mean-removed recording with Morlet(w0, f, fs).get_wavelet(), per epoch; truth is the float64 overlap-add convolution
of the oracle with that literal kernel, the metric conftest.rel_err (max |y - ref| / max |ref| per row), the gate the
project's 1e-5."""
import numpy as np
import pytest

from conftest import rel_err
from morlet_cases import truth as _truth

pytestmark = pytest.mark.gpu

TOL = 1e-5
CASES = [(6.0, 1000.0), (5.0, 1250.0), (10.0, 30000.0)]


def _as(output, c):
    return c if output == "complex" else np.abs(c) if output == "amplitude" else np.abs(c) ** 2


def _result(cwt, output):
    return {"amplitude": cwt.amplitude, "power": cwt.power, "complex": cwt.coefficients}[output]


def _report(name, err):
    print("%s: worst row %.2e (gate %.0e), median %.2e" % (name, np.max(err), TOL, np.median(err)))


def test_g16_through_the_class(golden):
    from ghost_amd.wave import ContinuousWaveletTransform, Morlet
    g = golden("G16_morlet.npz")
    cols = g["cols"]
    for w0, fs in CASES:
        tag = "%g_%g" % (w0, fs)
        f = g["frequencies_" + tag]
        cwt = ContinuousWaveletTransform(wavelet=Morlet(w0=w0))
        cwt.transform(g["x_" + tag], fs=fs, freqs=f, output="complex")
        order = np.argsort(f)                                # transform() sorts an explicit list upwards
        np.testing.assert_allclose(cwt.frequencies, f[order], rtol=1e-14)
        c = cwt.coefficients
        assert c.shape == (f.size, int(g["n"]))
        err = np.array([np.abs(c[i, cols] - g["conv_cols_%s_%d" % (tag, k)]).max() / float(g["rowmax_%s_%d" % (tag, k)])
                        for i, k in enumerate(order)])
        _report("G16 " + tag, err)
        assert err.max() <= TOL, (tag, err)


@pytest.mark.parametrize("output", ["amplitude", "power", "complex"])
@pytest.mark.parametrize("w0", [5.0, 6.0, 10.0])
def test_default_grid_every_row(w0, output):
    from ghost_amd.synthetic import lfp
    from ghost_amd.wave import ContinuousWaveletTransform, Morlet
    fs, n = 1000.0, 1 << 17
    x = lfp(2, n, fs, seed=11)
    cwt = ContinuousWaveletTransform(wavelet=Morlet(w0=w0))
    cwt.transform(x, fs=fs, multichannel=True, output=output)
    f = cwt.frequencies
    y = _result(cwt, output)
    assert y.shape == (2, f.size, n)
    si = cwt._plan.scale_info()
    assert (si["decimation"] >= 2).sum() > f.size // 2        # the fast path carries most of the grid
    for ch in range(2):
        err = rel_err(y[ch], _as(output, _truth(x[ch], fs, f, w0)))
        _report("w0=%g %s channel %d (%d rows)" % (w0, output, ch, f.size), err)
        assert err.max() <= TOL, (w0, output, ch, np.argmax(err), err.max())


def test_long_recording_levels_up_to_r16_and_beyond():
    """N = 1e6 at 1 kHz: the plan holds levels with R >= 16, which Morlet plans send through k_synth7's complex-gain
    instantiation (no interpolating synthesis).  A seeded subset of rows with at least one per decimation level and
    per method, amplitude and complex."""
    from ghost_amd.synthetic import lfp
    from ghost_amd.wave import ContinuousWaveletTransform, Morlet
    fs, n, w0 = 1000.0, 1000000, 6.0
    x = lfp(1, n, fs, seed=5)
    truth, rows = None, None
    for output in ("amplitude", "complex"):
        cwt = ContinuousWaveletTransform(wavelet=Morlet(w0=w0))
        cwt.transform(x[0], fs=fs, output=output, dtype=np.float32)
        f = cwt.frequencies
        si = cwt._plan.scale_info()
        assert f.size == 124 and si["decimation"].max() >= 16 and cwt._plan.info["n_interp"] == 0
        if rows is None:
            rng = np.random.default_rng(16)
            groups = {}
            for i, key in enumerate(zip(si["method"].tolist(), si["decimation"].tolist())):
                groups.setdefault(key, []).append(i)
            rows = sorted({int(rng.choice(v)) for v in groups.values()} | set(rng.choice(f.size, 4).tolist()))
            assert {(si["method"][r], si["decimation"][r]) for r in rows} == set(groups)
            truth = _truth(x[0], fs, f, w0, rows=rows)
        y = np.stack([cwt.fetch(scales=slice(r, r + 1))[0] for r in rows])
        err = rel_err(y, _as(output, truth))
        for r, e in zip(rows, err):
            print("1e6 %s row %3d %8.3f Hz method %d R %4d: %.2e" % (output, r, f[r], si["method"][r], si["decimation"][r], e))
        assert err.max() <= TOL, (output, err)


def test_two_epochs_with_a_gap():
    from ghost_amd.synthetic import lfp
    from ghost_amd.wave import ContinuousWaveletTransform, Morlet
    fs, w0 = 1000.0, 6.0
    n1, n2 = 30011, 41000
    x = lfp(1, n1 + n2, fs, seed=3)[0]
    t = np.concatenate([np.arange(n1) / fs, 100.0 + np.arange(n2) / fs])
    for output in ("complex", "amplitude"):
        cwt = ContinuousWaveletTransform(wavelet=Morlet(w0=w0))
        cwt.transform(x, fs=fs, timestamps=t, output=output)
        f = cwt.frequencies
        # the grid's lowest frequency comes from the shorter epoch
        assert Morlet(w0=w0, fs=fs).compute_lengths(f / 500.0 * np.pi).max() <= n1 // 5
        ref = _truth(x, fs, f, w0, bounds=[(0, n1), (n1, n1 + n2)])
        err = rel_err(_result(cwt, output), _as(output, ref))
        _report("two epochs " + output, err)
        assert err.max() <= TOL


def test_devices_sharding_is_bit_equal():
    from ghost_amd.synthetic import lfp
    from ghost_amd.wave import ContinuousWaveletTransform, Morlet
    x = lfp(3, 50000, 1000.0, seed=9)
    kw = dict(fs=1000.0, multichannel=True, dtype=np.float32)
    one = ContinuousWaveletTransform(wavelet=Morlet(w0=6)); one.transform(x, **kw)
    two = ContinuousWaveletTransform(wavelet=Morlet(w0=6)); two.transform(x, devices=[0, 0], **kw)
    np.testing.assert_array_equal(two.amplitude, one.amplitude)
    err = rel_err(one.amplitude[2], np.abs(_truth(x[2], 1000.0, one.frequencies, 6.0)))
    assert err.max() <= TOL


@pytest.mark.parametrize("output", ["amplitude", "complex"])
def test_output_stride_4(output):
    """Bit-equal to [..., ::4] of the full-rate call where the Morse tests demand it (tests/test_gpu_output_stride.py:
    the direct, block-convolution and full-band rows and every complex row); within the gate of the truth elsewhere."""
    from ghost_amd import _lib
    from ghost_amd.synthetic import lfp
    from ghost_amd.wave import ContinuousWaveletTransform, Morlet
    fs, w0 = 1000.0, 6.0
    x = lfp(1, 70001, fs, seed=4)[0]
    full = ContinuousWaveletTransform(wavelet=Morlet(w0=w0)); full.transform(x, fs=fs, output=output)
    strided = ContinuousWaveletTransform(wavelet=Morlet(w0=w0)); strided.transform(x, fs=fs, output=output, output_stride=4)
    a, b = _result(full, output)[..., ::4], _result(strided, output)
    assert a.shape == b.shape
    exact = strided._plan.scale_info()["method"] != _lib.SCALE_SPECTRAL
    if output == "complex":
        exact[:] = True
    assert exact.any()
    np.testing.assert_array_equal(b[exact], a[exact])
    ref = _as(output, _truth(x, fs, full.frequencies, w0))
    err = np.abs(b - ref[..., ::4]).max(axis=-1) / np.abs(ref).max(axis=-1)
    _report("output_stride=4 " + output, err)
    assert err.max() <= TOL


@pytest.mark.parametrize("precision", ["fast", "high", "auto", "exact"])
def test_precision_modes_on_a_benign_recording(precision):
    from ghost_amd.synthetic import lfp
    from ghost_amd.wave import ContinuousWaveletTransform, Morlet
    fs, w0 = 1000.0, 6.0
    x = lfp(1, 60000, fs, seed=8)[0]
    cwt = ContinuousWaveletTransform(wavelet=Morlet(w0=w0))
    cwt.transform(x, fs=fs, output="complex", precision=precision)
    err = rel_err(cwt.coefficients, _truth(x, fs, cwt.frequencies, w0))
    _report("precision=%s" % precision, err)
    assert err.max() <= TOL


def test_auto_watches_a_mains_line():
    from ghost_amd.synthetic import spectrum_class
    from ghost_amd.wave import ContinuousWaveletTransform, Morlet
    fs, w0 = 1000.0, 6.0
    x = spectrum_class("line100", 120000, fs)
    cwt = ContinuousWaveletTransform(wavelet=Morlet(w0=w0))
    cwt.transform(x, fs=fs, output="complex", precision="auto")
    assert cwt.precision_report["watched"]
    err = rel_err(cwt.coefficients, _truth(x, fs, cwt.frequencies, w0))
    _report("auto under line100 (rerouted %d)" % cwt.precision_report["rerouted"], err)
    assert err.max() <= TOL


def test_direct_kernel_is_get_wavelet(option):
    from ghost_amd import _lib
    from ghost_amd.engine import CwtPlan
    from ghost_amd.synthetic import lfp
    from ghost_amd.wave import Morlet
    fs = 1000.0
    for w0 in (5.0, 6.0, 10.0):
        if w0 == 10.0:                   # its shortest kernel has 59 taps: above the 48 the time domain takes by default
            option("direct_max_len", 128)
        hi = Morlet(w0=w0).compute_freq_bounds(50000)[1] / np.pi * fs / 2.0
        f = hi / 2 ** (np.arange(12) / 10.0)
        p = CwtPlan(50000, 1, fs, f, morlet_w0=w0, output="complex")
        p.execute(lfp(1, 50000, fs))
        direct = np.nonzero(p.scale_info()["method"] == _lib.SCALE_DIRECT)[0]
        assert direct.size > 0
        for s in direct:
            psi = Morlet(w0=w0, freq=f[s], fs=fs).get_wavelet()
            got = p.direct_kernel(int(s))
            assert got.shape == psi.shape
            # float64 taps rounded once to float32: half an ulp of each of the two components, 2^-24 of it, plus the float64
            # noise
            assert np.abs(got - psi).max() <= np.sqrt(2.0) * 2.0 ** -24 * np.abs(psi).max() * 1.01
        p.close()


def test_morse_after_morlet_and_back():
    from ghost_amd.synthetic import lfp
    from ghost_amd.wave import ContinuousWaveletTransform, Morlet, Morse
    fs = 1000.0
    x = lfp(1, 40000, fs, seed=2)[0]
    kw = dict(fs=fs, freqs=np.geomspace(150.0, 3.0, 20), dtype=np.float32)
    cwt = ContinuousWaveletTransform(wavelet=Morlet(w0=6))
    cwt.transform(x, **kw)
    first = cwt.amplitude.copy()
    key_morlet = cwt._plan_key
    cwt.wavelet = Morse(fs=fs)
    cwt.transform(x, **kw)
    assert cwt._plan_key != key_morlet
    fresh = ContinuousWaveletTransform(wavelet=Morse()); fresh.transform(x, **kw)
    np.testing.assert_array_equal(cwt.amplitude, fresh.amplitude)
    assert not np.array_equal(cwt.amplitude, first)
    cwt.wavelet = Morlet(w0=6, fs=fs)
    cwt.transform(x, **kw)
    assert cwt._plan_key == key_morlet
    np.testing.assert_array_equal(cwt.amplitude, first)
    other = ContinuousWaveletTransform(wavelet=Morlet(w0=7, fs=fs)); other.transform(x, **kw)
    assert other._plan_key != key_morlet and not np.array_equal(other.amplitude, first)
