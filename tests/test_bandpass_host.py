"""bandpass() without a GPU: the weights against quadrature and on the reference's own coefficients, the float64 model
and its derived bounds, band_rows, the C entry point's argument checks, the grid, and the refusals of the class and the
engine.  The device side: tests/test_gpu_bandpass.py."""
import ctypes as C
import math

import numpy as np
import pytest

import bandpass_model as bm
from oracle import ghost_oracle as orc

FS = 1000.0


def _morse(gamma, beta):
    from ghost_amd.wave.morse import Morse
    return Morse(fs=FS, gamma=gamma, beta=beta)


def _morlet(w0):
    from ghost_amd.wave.morlet import Morlet
    return Morlet(w0=w0, fs=FS)


# -- the weights ---------------------------------------------------------------------------------------------------------
def _cells(f):
    lf = np.log(np.asarray(f, dtype=np.float64))
    d = np.empty(lf.size)
    d[0], d[-1] = abs(lf[1] - lf[0]), abs(lf[-1] - lf[-2])
    d[1:-1] = np.abs(lf[2:] - lf[:-2]) / 2
    return d


@pytest.mark.parametrize("gamma,beta", [(3.0, 20.0), (3.0, 5.0), (3.0, 2.0), (2.0, 7.0)])
def test_morse_weights_are_the_cell_over_the_integral_of_the_response(gamma, beta):
    from ghost_amd.engine import band_weights
    f = np.geomspace(200.0, 4.0, 23)
    g, h = band_weights(f, _morse(gamma, beta))
    assert g.dtype == h.dtype == np.float32 and g.shape == h.shape == (23,)
    # the response with peak 2 at omega_p = (beta / gamma)^(1 / gamma), integrated over ln omega by the midpoint rule
    lw = (np.arange(1 << 18) + 0.5) * (24.0 / (1 << 18)) - 16.0
    om = np.exp(lw)
    psi = 2 * np.exp(beta * lw - om ** gamma - (beta / gamma) * (math.log(beta / gamma) - 1))
    assert abs(psi.max() - 2) < 1e-6
    c1, c2 = psi.sum() * 24.0 / (1 << 18), (psi ** 2).sum() * 24.0 / (1 << 18)
    np.testing.assert_allclose(g, 2 * _cells(f) / c1, rtol=1e-6)
    np.testing.assert_allclose(h, 4 * _cells(f) / c2, rtol=1e-6)


@pytest.mark.parametrize("w0", [6.0, 8.0, 5.0])
def test_morlet_weights_are_the_cell_over_the_integral_of_the_response(w0):
    from ghost_amd.engine import band_weights
    f = np.geomspace(4.0, 200.0, 17)                                      # ascending
    g, h = band_weights(f, _morlet(w0))
    sigma = (w0 + np.sqrt(2 + w0 ** 2)) * FS / (4 * np.pi * f)
    # another quadrature than the engine's: trapezoid in ln v
    lv = np.linspace(np.log(1e-9), np.log(w0 + 12.0), 400001)
    v = np.exp(lv)
    psi = np.exp(-0.5 * (v - w0) ** 2) - np.exp(-0.5 * w0 ** 2 - 0.5 * v ** 2)
    k1 = np.pi ** -0.25 * np.sqrt(2 * np.pi) * np.trapezoid(psi, lv)
    k2 = 2 * np.sqrt(np.pi) * np.trapezoid(psi ** 2, lv)
    np.testing.assert_allclose(g, 2 * _cells(f) / (np.sqrt(sigma) * k1), rtol=1e-6)
    np.testing.assert_allclose(h, 4 * _cells(f) / (sigma * k2), rtol=1e-6)


def test_cells_belong_to_the_grid():
    from ghost_amd.engine import band_weights
    wav = _morse(3.0, 20.0)
    f = np.array([100.0, 80.0, 50.0, 45.0, 10.0, 9.0])                     # not log-spaced
    g, h = band_weights(f, wav)
    np.testing.assert_allclose(g / g[0], _cells(f) / _cells(f)[0], rtol=1e-6)
    np.testing.assert_allclose(h / h[0], _cells(f) / _cells(f)[0], rtol=1e-6)
    gr, hr = band_weights(f[::-1], wav)                                     # ascending: the same cells, reversed
    assert np.array_equal(gr, g[::-1]) and np.array_equal(hr, h[::-1])
    g2, _ = band_weights(f[:2], wav)                                        # two rows: both one-sided
    assert g2[0] == g2[1] == g[0]
    assert np.all(g > 0) and np.all(h > 0)


def test_weights_refuse_what_has_no_cells():
    from ghost_amd.engine import band_weights
    wav = _morse(3.0, 20.0)
    for bad in ([10.0], [], 10.0):
        with pytest.raises(ValueError, match="at least 2"):
            band_weights(bad, wav)
    for bad in ([10.0, 20.0, 15.0], [10.0, 10.0, 20.0], [30.0, 20.0, 20.0]):
        with pytest.raises(ValueError, match="monotonic"):
            band_weights(bad, wav)
    for bad in ([10.0, np.nan], [0.0, 1.0], [-1.0, 1.0]):
        with pytest.raises(ValueError, match="finite and positive"):
            band_weights(bad, wav)
    for bad in (None, "morse", object()):
        with pytest.raises(ValueError, match="Morse and Morlet"):
            band_weights([10.0, 20.0], bad)


# -- the normalisation, on the reference's own coefficients -------------------------------------------------------------
# The grid is the one transform() makes for this recording when no limits are named: from the wavelet's own upper bound
# down, `voices` rows per octave.  Where the 20 Hz tone falls between two rows is then nobody's choice.  (At 4 voices the
# rows are 0.173 apart in ln f and the squared response of Morlet(8) is a Gaussian of sigma 0.088 there: the midpoint
# rule's error swings with that position inside +- 2 exp(-2 pi^2 sigma^2 / h^2) = 1.2 % -- 1.4 % with the tone exactly on
# a row, as on the grid 80 / 2^(j / 4) -- and is 0.9 % here.)
def _default_grid(wavelet, n, voices):
    lo, hi = np.asarray(wavelet.compute_freq_bounds(n)) / np.pi * FS / 2.0
    return hi / 2 ** (np.arange(np.floor(np.log2(hi / lo) * voices) + 1) / voices)


def _band_only(f, row):
    """(S, n) coefficients with the rows of 5 .. 80 Hz filled by row(r) -- the others are not read."""
    from ghost_amd.engine import band_rows
    first, count = band_rows((5.0, 80.0), f)[0]
    rows = [row(r) for r in range(first, first + count)]
    w = np.zeros((f.size, rows[0].size), np.complex128)
    w[first:first + count] = rows
    return w


def _reading(w, f, wavelet):
    """(envelope / A, power / A^2) of the band 5 .. 80 Hz in the middle of the recording."""
    from ghost_amd.engine import band_rows, band_weights
    g, h = band_weights(f, wavelet)
    rows = band_rows((5.0, 80.0), f)
    ref = bm.model(w[None], rows, g, h)
    mid = slice(w.shape[-1] // 2 - 256, w.shape[-1] // 2 + 256)
    return ref["envelope"][0, 0, mid] / 0.7, ref["power"][0, 0, mid] / 0.49


@pytest.mark.parametrize("voices", [10, 4])
@pytest.mark.parametrize("gamma,beta", [(3.0, 20.0), (3.0, 5.0)])
def test_a_tone_reads_its_amplitude_on_the_oracle(gamma, beta, voices):
    x = bm.tone()
    f = _default_grid(_morse(gamma, beta), x.size, voices)
    w = _band_only(f, lambda r: orc.cwt_complex(x, FS, f[r:r + 1], gamma=gamma, beta=beta)[0])
    env, pw = _reading(w, f, _morse(gamma, beta))
    print("Morse(%g, %g) %d voices: envelope / A %.4f .. %.4f, power / A^2 %.4f .. %.4f"
          % (gamma, beta, voices, env.min(), env.max(), pw.min(), pw.max()))
    assert np.all(np.abs(env - 1) < 0.01) and np.all(np.abs(pw - 1) < 0.01)


@pytest.mark.parametrize("voices", [10, 4])
@pytest.mark.parametrize("w0", [6.0, 8.0])
def test_a_tone_reads_its_amplitude_on_the_reference_morlet(w0, voices):
    from ghost_amd.wave.morlet import Morlet
    x = bm.tone()
    x = x - x.mean()
    f = _default_grid(_morlet(w0), x.size, voices)
    w = _band_only(f, lambda r: np.convolve(x, Morlet(w0=w0, freq=f[r], fs=FS).get_wavelet(), "same"))
    env, pw = _reading(w, f, _morlet(w0))
    print("Morlet(%g) %d voices: envelope / A %.4f .. %.4f, power / A^2 %.4f .. %.4f"
          % (w0, voices, env.min(), env.max(), pw.min(), pw.max()))
    assert np.all(np.abs(env - 1) < 0.01) and np.all(np.abs(pw - 1) < 0.01)


# -- the model ---------------------------------------------------------------------------------------------------------------
def test_bounds_are_the_derived_ones():
    u = 2.0 ** -24
    assert bm.U == u and bm.envelope_extra() == 2 * u
    for count in (1, 2, 9, 17, 23):
        assert bm.analytic_bound(count) == np.sqrt(2.0) * count * u
        assert bm.power_bound(count) == (2 + count) * u


def test_model_sums_are_the_definition():
    rng = np.random.default_rng(5)
    w = rng.standard_normal((2, 7, 40)) + 1j * rng.standard_normal((2, 7, 40))
    w[..., 10:17] = 0                                                       # a gap
    g, h = rng.standard_normal(7), rng.random(7)
    bands = [(0, 7), (2, 3), (3, 4), (6, 1), (0, 1), (2, 3)]               # overlapping, one-row, repeated
    ref = bm.model(w, bands, g, h)
    for k, (a, n) in enumerate(bands):
        z = sum(g[r] * w[:, r] for r in range(a, a + n))
        p = sum(h[r] * np.abs(w[:, r]) ** 2 for r in range(a, a + n))
        np.testing.assert_allclose(ref["analytic"][:, k], z, rtol=1e-13, atol=1e-15)
        np.testing.assert_allclose(ref["envelope"][:, k], np.abs(z), rtol=1e-13, atol=1e-15)
        np.testing.assert_allclose(ref["power"][:, k], p, rtol=1e-13, atol=1e-15)
        t = sum(abs(g[r]) * np.abs(w[:, r]) for r in range(a, a + n))
        np.testing.assert_allclose(bm.band_terms(w, bands, g)[:, k], t, rtol=1e-13)
    assert np.array_equal(ref["power"][:, 1], ref["power"][:, 5])
    for name in ("analytic", "envelope", "power"):
        assert ref[name].shape == (2, 6, 40) and not np.any(ref[name][..., 10:17])
    assert np.all(ref["envelope"][..., :10] > 0)


def test_the_float32_chains_of_the_model_meet_its_bounds():
    """chains32 is the prescribed order in NumPy; fmaf32 rounds once."""
    a = np.float32(1 + 2.0 ** -12)
    assert bm.fmaf32(a, a, np.float32(-1.0)) == np.float32(2.0 ** -11 + 2.0 ** -24)          # a * a alone would lose 2^-24
    assert bm.fmaf32(np.float32(3), np.float32(0), np.float32(0)) == 0
    # a * b = 2^-24 (1 - 2^-46), c = 1 + 2^-23: the exact sum lies just below the float32 tie and rounds to c; float64
    # rounds it onto the tie, from where a second rounding to nearest even would go up
    x, y, c = np.float32(2.0 ** -12 * (1 + 2.0 ** -23)), np.float32(2.0 ** -12 * (1 - 2.0 ** -23)), np.float32(1 + 2.0 ** -23)
    assert np.float32(np.float64(x) * np.float64(y) + np.float64(c)) == np.float32(1 + 2.0 ** -22)
    got = bm.fmaf32(x, np.array([y, -y]), c)
    assert got.dtype == np.float32 and got[0] == c
    assert got[1] == c and np.float32(np.float64(x) * -np.float64(y) + np.float64(c)) == 1   # just above the tie below c
    # against exact rational arithmetic, rounded once to 24 bits (ties to even); the third operand often nearly cancels
    from fractions import Fraction
    rng = np.random.default_rng(12)
    fa, fb = rng.standard_normal(600).astype(np.float32), rng.standard_normal(600).astype(np.float32)
    fc = np.where(rng.random(600) < 0.5, -(fa * fb) * (1 + rng.integers(-3, 4, 600) * 2.0 ** -23), rng.standard_normal(600))
    fc = fc.astype(np.float32)
    for a, b, c, got in zip(fa, fb, fc, bm.fmaf32(fa, fb, fc)):
        q = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
        want = 0.0
        if q:
            e = math.floor(math.log2(abs(q))) - 23
            while abs(q) >= Fraction(2) ** (e + 24):
                e += 1
            while abs(q) < Fraction(2) ** (e + 23):
                e -= 1
            want = float(round(q / Fraction(2) ** e) * Fraction(2) ** e)
        assert float(got) == want, (a, b, c, got, want)
    rng = np.random.default_rng(6)
    w = (rng.standard_normal((2, 23, 50)) + 1j * rng.standard_normal((2, 23, 50))).astype(np.complex64)
    w[..., 20:25] = 0
    g, h = rng.standard_normal(23).astype(np.float32), rng.random(23).astype(np.float32)
    bands = [(0, 23), (4, 1), (3, 2), (5, 9), (2, 17)]
    got, ref, t = bm.chains32(w, bands, g, h), bm.model(w, bands, g, h), bm.band_terms(w, bands, g)
    live = t > 0
    for k, (_, n) in enumerate(bands):
        m = live[:, k]
        ea = np.abs(got["analytic"][:, k] - ref["analytic"][:, k])
        assert np.all(ea[m] <= bm.analytic_bound(n) * t[:, k][m])
        ee = np.abs(got["envelope"][:, k] - ref["envelope"][:, k])
        assert np.all(ee[m] <= bm.analytic_bound(n) * t[:, k][m] + bm.envelope_extra() * ref["envelope"][:, k][m])
        ep = np.abs(got["power"][:, k] - ref["power"][:, k])
        assert np.all(ep[m] <= bm.power_bound(n) * ref["power"][:, k][m])
    for name in got:
        assert not np.any(got[name][..., 20:25])


def test_gate_bound_is_the_sum_of_what_each_row_may_move():
    rng = np.random.default_rng(8)
    w = rng.standard_normal((2, 5, 30)) + 1j * rng.standard_normal((2, 5, 30))
    g, h = rng.standard_normal(5), rng.random(5)
    bands = [(1, 3), (0, 5)]
    za, pw = bm.gate_bound(w, bands, g, h)
    eps = 1e-5 * np.abs(w).max(axis=-1)
    for k, (a, n) in enumerate(bands):
        np.testing.assert_allclose(za[:, k, 0], sum(abs(g[r]) * eps[:, r] for r in range(a, a + n)), rtol=1e-13)
        np.testing.assert_allclose(pw[:, k], sum(h[r] * (2 * np.abs(w[:, r]) * eps[:, r, None] + eps[:, r, None] ** 2)
                                                 for r in range(a, a + n)), rtol=1e-13)


# -- band_rows ---------------------------------------------------------------------------------------------------------
def test_band_rows_are_closed_intervals():
    from ghost_amd.engine import band_rows
    f = np.array([200.0, 100.0, 50.0, 25.0, 12.5])
    one = band_rows((25.0, 100.0), f)
    assert one.dtype == np.int32 and one.tolist() == [[1, 3]]
    assert band_rows([(25.0, 100.0)], f).tolist() == [[1, 3]]
    assert band_rows([[25.0, 100.0], (12.5, 12.5), (1, 1000), (26, 99)], f).tolist() == [[1, 3], [4, 1], [0, 5], [2, 1]]
    assert band_rows(np.array([[25.0, 100.0], [40.0, 60.0]]), f).tolist() == [[1, 3], [2, 1]]
    assert band_rows((25.0, 100.0), f[::-1]).tolist() == [[1, 3]]                      # ascending grids too
    assert band_rows(np.array([20.0, 120.0]), f).tolist() == [[1, 3]]


def test_band_rows_name_the_band_they_refuse():
    from ghost_amd.engine import band_rows
    f = np.array([200.0, 100.0, 50.0, 25.0, 12.5])
    for bad in ([], None, 5.0, "theta"):
        with pytest.raises(ValueError, match="bands"):
            band_rows(bad, f)
    for bad, k in (([(25, 100), (60, 40)], 1), ([(25, 100), (25, 100), (30, 40)], 2), ([(300, 400)], 0), ([(25, np.nan)], 0),
                   ([(25, 100), (25, 100, 3)], 1), ([(25, 100), "ab"], 1), ([(25, 100), (True, 30)], 1), ([(25, 100), 7.0], 1),
                   ([(25, 100), (np.inf, np.inf)], 1)):
        with pytest.raises(ValueError, match=r"bands\[%d\]" % k):
            band_rows(bad, f)
    with pytest.raises(ValueError, match=r"bands\[0\]"):
        band_rows((60, 40), f)
    with pytest.raises(ValueError, match=r"bands\[0\].*monotonic"):
        band_rows((20, 120), np.array([100.0, 10.0, 50.0]))


# -- the class and the engine: refusals that need no device --------------------------------------------------------------
def test_bandpass_before_any_transform_raises():
    from ghost_amd.wave import ContinuousWaveletTransform
    with pytest.raises(ValueError, match="transform"):
        ContinuousWaveletTransform().bandpass((4.0, 12.0))
    with pytest.raises(TypeError):
        ContinuousWaveletTransform().bandpass((4.0, 12.0), ("envelope",))              # keywords only
    with pytest.raises(TypeError):
        ContinuousWaveletTransform().bandpass()


def test_engine_bandpass_refuses_what_is_not_a_complex_device_result():
    from ghost_amd import engine
    from ghost_amd.multi import ShardedResult
    rows = np.array([[0, 2], [1, 2]], dtype=np.int32)
    g = h = np.ones(3, np.float32)
    with pytest.raises(ValueError, match="one device"):
        engine.bandpass(ShardedResult([], (4, 3, 100), True), rows, g, h)
    with pytest.raises(ValueError, match="complex"):
        engine.bandpass(engine.DeviceResult(object(), (4, 3, 100), 128, False), rows, g, h)
    with pytest.raises(ValueError, match="freed"):
        engine.bandpass(engine.DeviceResult(None, (4, 3, 100), 128, True), rows, g, h)
    stub = engine.DeviceResult(object(), (4, 3, 100), 128, True)
    for bad in ((), ("phase",), ("power", "power"), None, 3, ("power", 3), ""):
        with pytest.raises(ValueError, match="outputs"):
            engine.bandpass(stub, rows, g, h, bad)
    for bad in ([], [0, 2], [[0, 2, 1]], [[0.0, 2.0]], [[True, True]]):
        with pytest.raises(ValueError, match="rows"):
            engine.bandpass(stub, np.array(bad), g, h)
    for bad, k in (([[0, 0]], 0), ([[0, 3], [-1, 2]], 1), ([[0, 3], [0, 3], [2, 2]], 2), ([[0, 4]], 0)):
        with pytest.raises(ValueError, match=r"rows\[%d\]" % k):
            engine.bandpass(stub, np.array(bad), g, h)
    for bad in (np.ones(2, np.float32), np.ones((3, 1)), None, np.array([1.0, np.nan, 1.0]), np.array([1.0, np.inf, 1.0]),
                np.ones(3, bool), np.ones(3, complex)):
        with pytest.raises(ValueError, match="'g'"):
            engine.bandpass(stub, rows, bad, h)
        with pytest.raises(ValueError, match="'h'"):
            engine.bandpass(stub, rows, g, bad)
    with pytest.raises(ValueError, match="'h'.*at least 0"):
        engine.bandpass(stub, rows, g, np.array([1.0, -1e-9, 1.0]))
    with pytest.raises(ValueError, match="'h'"):                                       # g is not looked at for power alone
        engine.bandpass(stub, rows, None, None, ("power",))
    with pytest.raises(ValueError, match="'g'"):
        engine.bandpass(stub, rows, None, None, ("envelope",))


def test_class_bandpass_refuses_results_it_cannot_use():
    from ghost_amd import engine
    from ghost_amd.multi import ShardedResult
    from ghost_amd.wave import ContinuousWaveletTransform
    cwt = ContinuousWaveletTransform()
    cwt._frequencies, cwt._fs = np.geomspace(100.0, 10.0, 3), FS
    cwt._device_result, cwt._pending = engine.DeviceResult(object(), (1, 3, 100), 128, False), ("amplitude", np.float32, True)
    with pytest.raises(ValueError, match="output='complex'"):
        cwt.bandpass((10.0, 100.0))
    cwt._device_result, cwt._pending = ShardedResult([], (4, 3, 100), True), ("complex", np.float32, False)
    with pytest.raises(ValueError, match="sharded"):
        cwt.bandpass((10.0, 100.0))
    cwt._device_result = engine.DeviceResult(None, (1, 3, 100), 128, True)
    with pytest.raises(ValueError, match="freed"):
        cwt.bandpass((10.0, 100.0))
    cwt._device_result = engine.DeviceResult(object(), (1, 3, 100), 128, True)
    with pytest.raises(ValueError, match=r"bands\[1\]"):
        cwt.bandpass([(10.0, 100.0), (200.0, 300.0)])
    with pytest.raises(ValueError, match="outputs"):
        cwt.bandpass((10.0, 100.0), outputs=("phase",))
    cwt._device_result = None


# -- the C entry point: arguments first, then the device ----------------------------------------------------------------
def test_entry_point_validates_then_needs_a_device():
    from ghost_amd import _lib
    from ghost_amd.engine import device_count
    lib = _lib.lib
    buf = (C.c_float * 256)()
    good = (C.c_int32 * 4)(0, 4, 1, 2)
    ones = (C.c_float * 4)(1.0, -2.0, 0.0, 3.0)
    pos = (C.c_float * 4)(1.0, 2.0, 0.0, 3.0)

    def call(rows=buf, pitch=16, c=1, s=4, n=16, bands=good, n_b=2, g=ones, h=pos, ana=buf, env=buf, pw=buf, out_pitch=16):
        return lib.gcwt_bandpass(rows, pitch, c, s, n, bands, n_b, g, h, ana, env, pw, out_pitch)

    def f4(*v):
        return (C.c_float * 4)(*v)

    for kw, word in ((dict(rows=None), b"d_rows is NULL"), (dict(bands=None), b"bands is NULL"), (dict(g=None), b"g is NULL"),
                     (dict(g=None, ana=None), b"g is NULL"), (dict(h=None), b"h is NULL"), (dict(c=0), b"n_channels"),
                     (dict(s=0), b"n_scales"), (dict(n=0), b"n_cols"), (dict(pitch=15), b"pitch"), (dict(n_b=0), b"n_bands"),
                     (dict(n_b=-1), b"n_bands"), (dict(bands=(C.c_int32 * 4)(0, 4, -1, 2)), b"band 1"),
                     (dict(bands=(C.c_int32 * 4)(0, 0, 1, 2)), b"band 0"), (dict(bands=(C.c_int32 * 4)(0, 4, 3, 2)), b"band 1"),
                     (dict(bands=(C.c_int32 * 4)(0, 5, 1, 2)), b"band 0"), (dict(bands=(C.c_int32 * 4)(0, 4, 4, 1)), b"band 1"),
                     (dict(bands=(C.c_int32 * 4)(0, 4, 2**31 - 1, 2**31 - 1)), b"band 1"),
                     (dict(g=f4(1, float("nan"), 0, 0)), b"g[1]"), (dict(g=f4(1, 1, 1, float("inf"))), b"g[3]"),
                     (dict(h=f4(float("-inf"), 1, 1, 1)), b"h[0]"), (dict(h=f4(1, 1, -1e-30, 1)), b"h[2]"),
                     (dict(h=f4(1, float("nan"), 1, 1)), b"h[1]"), (dict(out_pitch=15), b"out_pitch"),
                     (dict(ana=None, env=None, pw=None), b"nothing"),
                     (dict(c=2**31 - 1, n=2**40, pitch=2**40, out_pitch=2**40), b"workgroups"),
                     (dict(c=2**20, n=2**21, pitch=2**21, out_pitch=2**21), b"workgroups")):
        assert call(**kw) == _lib.ERR_INVALID, kw
        msg = lib.gcwt_last_error()
        assert msg.startswith(b"gcwt_bandpass:") and word in msg, (kw, msg)
    # a valid request: without a GPU there is nothing that computes it; with one, host memory is not a resident result
    n_dev = device_count()
    for kw in (dict(), dict(g=None, ana=None, env=None), dict(h=None, pw=None), dict(h=None, pw=None, env=None), dict(n_b=1),
               dict(n=15), dict(bands=(C.c_int32 * 4)(3, 1, 0, 1)), dict(g=f4(-1, -1, -1, -1), h=f4(0, 0, 0, 0))):
        rc = call(**kw)
        if n_dev == 0:
            assert rc == _lib.ERR_NO_DEVICE and b"no CPU path" in lib.gcwt_last_error(), kw
        else:
            assert rc == _lib.ERR_INVALID and b"device memory" in lib.gcwt_last_error(), kw


# -- the grid ------------------------------------------------------------------------------------------------------------
def _grid(c, n, n_b):
    from ghost_amd import _lib
    ct, blocks = C.c_int64(), C.c_int64()
    grp = C.c_int32()
    rc = _lib.lib.gcwt_debug_bandpass_grid(c, n, n_b, C.byref(ct), C.byref(grp), C.byref(blocks))
    assert rc == 0, _lib.lib.gcwt_last_error()
    return ct.value, grp.value, blocks.value


def test_grid_covers_every_tile_of_every_channel_once():
    """The kernel's own index arithmetic (resident_op.h: shared_place), replayed over the whole grid: every (channel,
    column tile, band group) is some workgroup's, exactly once, and the rest is the padding that returns at once."""
    from ghost_amd import _lib
    lib = _lib.lib
    t, grp_bands = 512, 4                                                   # GCWT_BANDPASS_TILE_COLS, GCWT_BANDPASS_GROUP_BANDS
    for c in (1, 8, 9):
        for n in (1, t - 1, t, t + 1, 2 * t + 3):
            for n_b in (1, grp_bands, grp_bands + 1, 2 * grp_bands + 1):
                ct, grp, blocks = _grid(c, n, n_b)
                assert (ct, grp) == (-(-n // t), -(-n_b // grp_bands)), (c, n, n_b)
                units = c * ct
                assert blocks == -(-units // 8) * 8 * grp and blocks < 2 ** 31
                idx = np.arange(blocks)
                member, rest = idx % 8, idx // 8
                tile, unit = rest % grp, rest // grp * 8 + member
                live = unit < units
                cells = np.stack((unit[live] // ct, unit[live] % ct, tile[live]), axis=1)
                assert len(cells) == c * ct * grp and len(np.unique(cells, axis=0)) == len(cells)
                assert cells[:, 0].max() == c - 1 and cells[:, 1].max() == ct - 1 and cells[:, 2].max() == grp - 1
                # the columns and bands of the tiles: every column and every band once
                assert (ct - 1) * t < n <= ct * t and (grp - 1) * grp_bands < n_b <= grp * grp_bands
    assert _grid(1, 512, 4) == (1, 1, 8) and _grid(1, 513, 5) == (2, 2, 16)
    assert _grid(128, 1000000, 2) == (1954, 1, 128 * 1954)
    assert lib.gcwt_debug_bandpass_grid(1, 512, 4, None, None, None) == 0
    for c, n, n_b in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 1, 1), (2**20, 2**21, 1), (2**31 - 1, 2**62, 2**31 - 1)):
        assert lib.gcwt_debug_bandpass_grid(c, n, n_b, None, None, None) == _lib.ERR_INVALID, (c, n, n_b)
