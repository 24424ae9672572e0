"""ridge() without a GPU: the weights against the wavelets' own responses, the two models of the definition against each
other and on planted cases, the physical reading and the chirp on the reference's own coefficients, grid_frequency(), the C
entry point's argument checks, and the refusals of the class and the engine.  The device side: tests/test_gpu_ridge.py."""
import ctypes as C

import numpy as np
import pytest

import ridge_model as rm
from oracle import ghost_oracle as orc

FS = 1000.0


def _morse(gamma=3.0, beta=20.0):
    from ghost_amd.wave.morse import Morse
    return Morse(fs=FS, gamma=gamma, beta=beta)


def _morlet(w0):
    from ghost_amd.wave.morlet import Morlet
    return Morlet(w0=w0, fs=FS)


# -- the weights ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gamma,beta", [(3.0, 20.0), (3.0, 5.0), (2.0, 7.0)])
def test_morse_weights_are_the_inverse_square_of_the_kernels_gain(gamma, beta):
    from ghost_amd.engine import ridge_weights
    f = np.geomspace(120.0, 6.0, 9)
    e = ridge_weights(f, _morse(gamma, beta))
    assert e.dtype == np.float32 and e.shape == (9,) and np.all(e == 1)
    # the literal kernel of every row (what the reference convolves with), its response at the row's own frequency: a
    # sinusoid of amplitude A is two exponentials of A / 2
    omega = orc.hz_to_rad(f, FS)
    for r, length in enumerate(orc.morse_lengths(omega, gamma, beta)):
        kernel, _ = orc.morse_kernel(length, omega[r], gamma, beta)
        gain = 0.5 * abs(np.sum(kernel * np.exp(-1j * omega[r] * np.arange(length))))
        assert abs(e[r] * gain ** 2 - 1) < 1e-3, (r, gain)


@pytest.mark.parametrize("w0", [6.0, 8.0, 5.0])
def test_morlet_weights_are_the_inverse_square_of_the_kernels_gain(w0):
    from ghost_amd.engine import ridge_weights
    from ghost_amd.wave.morlet import Morlet
    f = np.geomspace(4.0, 150.0, 11)                                      # ascending
    e = ridge_weights(f, _morlet(w0))
    assert e.dtype == np.float32 and e.shape == (11,)
    for r in range(f.size):
        kernel = Morlet(w0=w0, freq=f[r], fs=FS).get_wavelet()
        gain = 0.5 * abs(np.sum(kernel * np.exp(-2j * np.pi * f[r] / FS * np.arange(kernel.size))))
        assert abs(e[r] * gain ** 2 - 1) < 1e-5, (r, gain, e[r])
    assert np.all(np.diff(e) > 0)                                          # energy-normalised rows: the gain falls with f
    assert np.array_equal(ridge_weights(f[::-1], _morlet(w0)), e[::-1])


def test_weights_refuse_what_they_do_not_know():
    from ghost_amd.engine import ridge_weights
    for bad in ([], [10.0, np.nan], [0.0, 1.0], [-1.0, 1.0], [np.inf]):
        with pytest.raises(ValueError, match="at least 1|finite and positive"):
            ridge_weights(bad, _morse())
    for bad in (None, "morse", object()):
        with pytest.raises(ValueError, match="Morse and Morlet"):
            ridge_weights([10.0, 20.0], bad)
    assert ridge_weights(10.0, _morse()).shape == (1,)


# -- the models ----------------------------------------------------------------------------------------------------------
def _random(c, s, n, seed):
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((c, s, n)) + 1j * rng.standard_normal((c, s, n))).astype(np.complex64)
    w[..., n // 3:n // 3 + n // 5] = 0
    return w, (0.5 + rng.random(s)).astype(np.float32), (2.5 * np.pi * rng.random(s)).astype(np.float32)


def test_the_float32_model_is_the_definition_up_to_rounding():
    w, e, nu = _random(2, 11, 400, 3)
    bands = [(0, 11), (4, 1), (3, 2), (2, 7), (9, 2)]
    seg = [(0, 100), (100, 101), (101, 150), (150, 400)]
    ref, got = rm.model(w, bands, e, nu, 250.0, seg), rm.ranking32(w, bands, e)
    q = e.astype(np.float64)[None, :, None] * np.abs(w.astype(np.complex128)) ** 2
    tie = rm.near_ties(q, bands, 1e-6)
    assert tie.mean() < 0.5                                                # (the gap columns are ties at 0)
    gap = slice(400 // 3, 400 // 3 + 80)
    assert np.all(got["row"][..., gap] == -1) and not np.any(got["amplitude"][..., gap]) and not np.any(got["offset"][..., gap])
    assert np.all(np.isnan(ref["frequency"][..., gap])) and np.all(ref["row"][..., gap] == -1)
    live = np.ones(400, bool)
    live[gap] = False
    assert np.all(got["row"][..., live] >= 0)
    same = ~tie
    assert np.array_equal(got["row"][same], ref["row"][same])
    assert np.all(np.abs(got["amplitude"] - ref["amplitude"])[same] <= 3 * rm.U * ref["amplitude"][same])
    for k, (a, cnt) in enumerate(bands):
        assert np.all((got["row"][:, k] == -1) | ((got["row"][:, k] >= a) & (got["row"][:, k] < a + cnt)))
        edge = (got["row"][:, k] == a) | (got["row"][:, k] == a + cnt - 1)
        assert not np.any(got["offset"][:, k][edge])
    assert np.all(np.abs(ref["offset"]) <= 0.5) and np.any(ref["offset"] != 0)
    # the offset divides two differences of nearly equal numbers: compare where the parabola is well conditioned
    steep = same & (np.abs(got["offset"].astype(np.float64) - ref["offset"]) > 1e-3)
    assert steep.mean() < 0.01
    # no frequency in the one-column segment, in the gap and beside it (a neighbour that is 0 has no phase); everywhere else
    none = ~live
    none[[100, gap.start - 1, gap.stop]] = True
    assert np.array_equal(np.isnan(ref["frequency"]), np.broadcast_to(none, ref["frequency"].shape))
    # the prescribed product against the exact one: within Z_ANGLE
    re, im, span = rm.product32(w, got["row"], seg)
    assert span[0] == 1 and span[99] == 1 and span[100] == 0 and span[101] == 1 and span[50] == 2 and span[399] == 1
    f64 = rm.frequency64(w, got["row"], nu, 250.0, seg)
    ok = ~np.isnan(f64["frequency"])
    d = np.angle((re + 1j * im.astype(np.float64)) * np.exp(-1j * f64["angle"]))
    assert np.abs(d[ok]).max() <= rm.Z_ANGLE
    assert np.any(f64["k"][ok] != 0)                                        # nu reaches past pi: the unwrapping is at work


def test_planted_ties_edges_and_a_flat_parabola():
    e = np.ones(6, np.float32)
    w = np.zeros((1, 6, 8), np.complex64)
    w[0, :, 0] = [1, 2, 2, 1, 2, 0]                                         # equal maxima: the lowest index wins
    w[0, :, 1] = [3, 1, 1, 1, 1, 1]                                         # the band's first row
    w[0, :, 2] = [1, 1, 1, 1, 1, 3]                                         # ... and its last
    w[0, :, 3] = [0, 1, 3, 2, 0, 0]                                         # a plain parabola: q = 1, 9, 4
    w[0, :, 4] = [0, 0, 0, 0, 0, 0]                                         # a gap
    w[0, :, 5] = [1j, 1j, 1j, 1j, 1j, 1j]                                   # all equal: row 0
    w[0, :, 6] = [0, 0, 0, 2, 0, 0]
    w[0, :, 7] = [0, 0, 1, 1, 0, 0]
    got = rm.ranking32(w, [(0, 6), (1, 4)], e)
    assert got["row"][0, 0].tolist() == [1, 0, 5, 2, -1, 0, 3, 2]
    assert got["row"][0, 1].tolist() == [1, 1, 1, 2, -1, 1, 3, 2]
    assert got["amplitude"][0, 0].tolist() == [2, 3, 3, 3, 0, 1, 2, 1]
    off = got["offset"][0, 0]
    assert off[0] == np.float32(0.5 * (1 - 4) / (1 + 4 - 8)) == 0.5 and off[1] == 0 and off[2] == 0 and off[4] == 0 and off[5] == 0
    assert off[3] == np.float32(np.float32(0.5 * (1 - 4)) / np.float32(1 + 4 - 18)) and off[6] == 0 and off[7] == 0.5
    assert got["offset"][0, 1].tolist()[:3] == [0, 0, 0]                    # row 1 is that band's first
    # d2 == 0: qm = 1 - 2^-24, q = qp = 1: qm + qp rounds to 2 and the denominator vanishes
    e2 = np.array([1 - 2.0 ** -24, 1, 1], np.float32)
    w2 = np.ones((1, 3, 1), np.complex64)
    flat = rm.ranking32(w2, [(0, 3)], e2)
    assert flat["row"][0, 0, 0] == 1 and flat["offset"][0, 0, 0] == 0 and not np.signbit(flat["offset"][0, 0, 0])
    assert rm.model(w2, [(0, 3)], e2, np.zeros(3), 1.0, [(0, 1)])["offset"][0, 0, 0] == 0.5


def test_frequency_unwraps_against_the_rows_own_advance():
    """A row that turns by theta per column reads theta / (2 pi) cycles per column whatever the stride: with nu near
    theta the integer k restores the turns that the arctangent cannot see."""
    n = 64
    for theta in (0.3, 3.0, 7.0, 2 * np.pi * 3.2):
        w = np.zeros((1, 3, n), np.complex128)
        w[0, 1] = 0.7 * np.exp(1j * (theta * np.arange(n) + 0.2))
        nu = np.array([0.0, theta * 1.02, 0.0])
        f = rm.frequency64(w, np.ones((1, 1, n), np.int32), nu, 250.0, [(0, 31), (31, n)])
        np.testing.assert_allclose(f["frequency"], theta / (2 * np.pi) * float(np.float32(250.0)), rtol=1e-12)
        assert np.all(f["k"][0, 0, 1:30] == np.rint((2 * theta) / (2 * np.pi) - np.angle(np.exp(2j * theta)) / (2 * np.pi)))
        assert f["span"].tolist() == [1] + [2] * 29 + [1, 1] + [2] * 31 + [1]
    none = rm.frequency64(w, np.full((1, 1, n), -1, np.int32), nu, 250.0, [(0, n)])
    assert np.all(np.isnan(none["frequency"]))
    w[0, 1, 10] = 0                                                         # a zero neighbour: columns 9 and 11 have no angle
    hole = np.isnan(rm.frequency64(w, np.ones((1, 1, n), np.int32), nu, 250.0, [(0, n)])["frequency"][0, 0])
    assert np.flatnonzero(hole).tolist() == [9, 11]


def test_the_frequency_bound_is_the_counted_one():
    u = 2.0 ** -24
    assert rm.U == u and rm.Z_ANGLE == 2 * np.sqrt(2.0) * u and rm.ATAN_GATE == 2 * rm.ATAN_WORST <= 2e-6
    for angle, k, span, hz in ((0.5, 0, 2, 1000.0), (-3.0, 3, 1, 250.0)):
        want = hz / (2 * np.pi * span) * (rm.Z_ANGLE + rm.ATAN_GATE + 2 * u * 2 * np.pi * abs(k) + 4 * u * abs(angle + 2 * np.pi * k))
        assert abs(rm.frequency_bound(angle, k, span, hz) / want - 1) <= 2 * rm.SECOND_ORDER


# -- the physical reading, on the reference's own coefficients -------------------------------------------------------------
def _reads(w, f, wavelet, f0, amplitude):
    from ghost_amd.engine import ridge_weights
    e = ridge_weights(f, wavelet)
    n = w.shape[-1]
    ref = rm.model(w[None], [(0, f.size)], e, 2 * np.pi * f / FS, FS, [(0, n)])
    mid = slice(n // 2 - 256, n // 2 + 256)
    assert np.all(ref["row"][0, 0, mid] == int(np.argmin(np.abs(f - f0))))
    return ref["amplitude"][0, 0, mid] / amplitude, ref["frequency"][0, 0, mid] / f0, ref["offset"][0, 0, mid]


@pytest.mark.parametrize("gamma,beta", [(3.0, 20.0), (3.0, 5.0)])
def test_a_tone_on_a_row_reads_its_amplitude_and_frequency_on_the_oracle(gamma, beta):
    f0, amp = 20.0, 0.7
    f = f0 * 2.0 ** (np.arange(4, -5, -1) / 10.0)                           # 10 voices per octave, the tone on row 4
    x = amp * np.cos(2 * np.pi * f0 * np.arange(8192) / FS + 0.3)
    w = orc.cwt_complex(x, FS, f, gamma=gamma, beta=beta)
    a, fr, off = _reads(w, f, _morse(gamma, beta), f0, amp)
    print("Morse(%g, %g): amplitude / A %.6f .. %.6f, frequency / f %.8f .. %.8f, offset %.4f .. %.4f"
          % (gamma, beta, a.min(), a.max(), fr.min(), fr.max(), off.min(), off.max()))
    assert np.all(np.abs(a - 1) < 1e-5) and np.all(np.abs(fr - 1) < 1e-6) and np.all(np.abs(off) < 0.05)


@pytest.mark.parametrize("w0", [6.0, 8.0])
def test_a_tone_on_a_row_reads_its_amplitude_and_frequency_on_the_reference_morlet(w0):
    from ghost_amd.wave.morlet import Morlet
    f0, amp = 20.0, 0.7
    f = f0 * 2.0 ** (np.arange(-4, 5) / 10.0)                               # ascending
    x = amp * np.cos(2 * np.pi * f0 * np.arange(8192) / FS + 0.3)
    x = x - x.mean()
    w = np.stack([np.convolve(x, Morlet(w0=w0, freq=fr, fs=FS).get_wavelet(), "same") for fr in f])
    a, fr, off = _reads(w, f, _morlet(w0), f0, amp)
    print("Morlet(%g): amplitude / A %.6f .. %.6f, frequency / f %.8f .. %.8f, offset %.4f .. %.4f"
          % (w0, a.min(), a.max(), fr.min(), fr.max(), off.min(), off.max()))
    # e levels the rows' gains, each at its own frequency; the levelled response to one tone, as a function of the row, then
    # peaks where sigma_r omega = w0, not at the row whose peak frequency is the tone's (sigma_r omega = (w0 + sqrt(2 + w0^2))
    # / 2): `offset` and grid_frequency() read log2 of that ratio x 10 rows high (1.4 % at w0 = 6); `frequency` does not
    lean = 10 * np.log2((w0 + np.sqrt(2 + w0 ** 2)) / (2 * w0))
    assert np.all(np.abs(a - 1) < 1e-5) and np.all(np.abs(fr - 1) < 1e-6) and np.all(np.abs(off - lean) < 0.03), lean
    # without the weights the energy-normalised rows lean to low frequencies: the unweighted maximum sits a row lower
    flat = rm.model(w[None], [(0, f.size)], np.ones(f.size), 2 * np.pi * f / FS, FS, [(0, x.size)])
    assert np.all(flat["offset"][0, 0, 4000:4200] < off[:200])


def test_the_chirp_has_few_near_ties_on_the_oracle():
    """The condition of the end-to-end test on the device (tests/test_gpu_ridge.py): on the oracle's coefficients at most
    1 % of the columns have their two largest q within 4e-5 of each other -- four times the transform's 1e-5 gate on each
    of the two rows -- and the ridge follows the sweep."""
    x = rm.chirp()
    f = rm.CHIRP_FREQS
    w = orc.cwt_complex(x, FS, f)
    q = np.abs(w[None]) ** 2
    bands = [(0, f.size), (0, 16), (3, 16)]                                 # 20 .. 100, 20 .. 76 and 26 .. 100 Hz: the sweep inside
    tie = rm.near_ties(q, bands)
    print("near ties: %s of %d columns" % (tie.sum(axis=-1).ravel().tolist(), x.size))
    assert tie.mean(axis=-1).max() <= 0.01
    ref = rm.model(w[None], bands, np.ones(f.size), 2 * np.pi * f / FS, FS, [(0, x.size)])
    mid = slice(1500, x.size - 1500)
    inst = 31.0 + (67.0 - 31.0) * np.arange(x.size) / x.size                 # the sweep's instantaneous frequency
    assert np.all(np.abs(ref["frequency"][0, 0, mid] / inst[mid] - 1) < 0.01)
    assert np.all(np.abs(ref["amplitude"][0, 0, mid] / 0.8 - 1) < 0.06)     # (between two rows a sweep reads up to 5 % low)
    assert np.all(np.diff(ref["row"][0, 0, mid]) >= 0) and ref["row"][0, 0, mid].min() < ref["row"][0, 0, mid].max()


# -- grid_frequency() ----------------------------------------------------------------------------------------------------
def test_grid_frequency_interpolates_ln_f():
    from ghost_amd.wave.transforms import _Ridge
    f = np.array([80.0, 40.0, 20.0, 10.0])
    row = np.array([[[1, 1, 1, 3, -1, 0]]], np.int32)
    off = np.array([[[0.0, 0.5, -0.25, 0.0, 0.0, 0.0]]], np.float32)
    r = _Ridge(row, None, None, off, None, None, None, None, f)
    got = r.grid_frequency()
    assert got.shape == row.shape and got.dtype == np.float64
    np.testing.assert_allclose(got[0, 0, :4], [40.0, 40.0 / 2 ** 0.5, 40.0 * 2 ** 0.25, 10.0], rtol=1e-12)
    assert np.isnan(got[0, 0, 4]) and abs(got[0, 0, 5] - 80.0) < 1e-12
    for r in (_Ridge(None, None, None, off, None, None, None, None, f), _Ridge(row, None, None, None, None, None, None, None, f)):
        with pytest.raises(ValueError, match="row.*offset"):
            r.grid_frequency()


# -- the class and the engine: refusals that need no device --------------------------------------------------------------
def test_ridge_before_any_transform_raises():
    from ghost_amd.wave import ContinuousWaveletTransform
    with pytest.raises(ValueError, match="transform"):
        ContinuousWaveletTransform().ridge((4.0, 12.0))
    with pytest.raises(TypeError):
        ContinuousWaveletTransform().ridge((4.0, 12.0), ("row",))             # keywords only
    with pytest.raises(TypeError):
        ContinuousWaveletTransform().ridge()


def test_engine_ridge_refuses_what_it_cannot_use():
    from ghost_amd import engine
    from ghost_amd.multi import ShardedResult
    rows = np.array([[0, 2], [1, 2]], dtype=np.int32)
    e, nu, seg = np.ones(3, np.float32), np.zeros(3, np.float32), np.array([[0, 40], [40, 100]])
    with pytest.raises(ValueError, match="one device"):
        engine.ridge(ShardedResult([], (4, 3, 100), True), rows, e, nu, 1000.0, seg)
    with pytest.raises(ValueError, match="complex"):
        engine.ridge(engine.DeviceResult(object(), (4, 3, 100), 128, False), rows, e, nu, 1000.0, seg)
    with pytest.raises(ValueError, match="freed"):
        engine.ridge(engine.DeviceResult(None, (4, 3, 100), 128, True), rows, e, nu, 1000.0, seg)
    stub = engine.DeviceResult(object(), (4, 3, 100), 128, True)
    for bad in ((), ("phase",), ("row", "row"), None, 3, ("row", 3), "", ("envelope",)):
        with pytest.raises(ValueError, match="outputs"):
            engine.ridge(stub, rows, e, nu, 1000.0, seg, bad)
    for bad in ([], [0, 2], [[0, 2, 1]], [[0.0, 2.0]], [[True, True]]):
        with pytest.raises(ValueError, match="rows"):
            engine.ridge(stub, np.array(bad), e, nu, 1000.0, seg)
    for bad, k in (([[0, 0]], 0), ([[0, 3], [-1, 2]], 1), ([[0, 3], [0, 3], [2, 2]], 2), ([[0, 4]], 0)):
        with pytest.raises(ValueError, match=r"rows\[%d\]" % k):
            engine.ridge(stub, np.array(bad), e, nu, 1000.0, seg)
    for bad in (np.ones(2, np.float32), np.ones((3, 1)), None, np.array([1.0, np.nan, 1.0]), np.array([1.0, np.inf, 1.0]),
                np.ones(3, bool), np.ones(3, complex), np.array([1.0, -1.0, 1.0])):
        with pytest.raises(ValueError, match="'e'"):
            engine.ridge(stub, rows, bad, nu, 1000.0, seg)
        with pytest.raises(ValueError, match="'nu'"):
            engine.ridge(stub, rows, e, bad, 1000.0, seg)
    with pytest.raises(ValueError, match="'e'.*above 0"):
        engine.ridge(stub, rows, np.array([1.0, 0.0, 1.0]), nu, 1000.0, seg)
    with pytest.raises(ValueError, match="'e'.*above 0"):
        engine.ridge(stub, rows, np.array([1.0, 1e-60, 1.0]), nu, 1000.0, seg)    # 0 in float32
    for bad in (0.0, -1.0, np.nan, np.inf, 1e60, None, "1000", True):
        with pytest.raises(ValueError, match="hz_per_cycle"):
            engine.ridge(stub, rows, e, nu, bad, seg)
    for bad in ([], [0, 100], [[0, 50, 100]], [[0.0, 100.0]], [[True, True]], None):
        with pytest.raises(ValueError, match="'segments'"):
            engine.ridge(stub, rows, e, nu, 1000.0, np.array(bad) if bad is not None else None)
    for bad, k in (([[0, 0], [0, 100]], 0), ([[1, 100]], 0), ([[0, 40], [41, 100]], 1), ([[0, 40], [39, 100]], 1),
                   ([[0, 40], [40, 101]], 1), ([[0, 40], [40, 90]], 1), ([[0, 40], [40, 30]], 1), ([[-1, 100]], 0)):
        with pytest.raises(ValueError, match=r"segments\[%d\]" % k):
            engine.ridge(stub, rows, e, nu, 1000.0, np.array(bad))


def test_class_ridge_refuses_results_it_cannot_use():
    from ghost_amd import engine
    from ghost_amd.multi import ShardedResult
    from ghost_amd.wave import ContinuousWaveletTransform
    cwt = ContinuousWaveletTransform()
    cwt._frequencies, cwt._fs = np.geomspace(100.0, 10.0, 3), FS
    cwt._device_result, cwt._pending = engine.DeviceResult(object(), (1, 3, 100), 128, False), ("amplitude", np.float32, True)
    with pytest.raises(ValueError, match="output='complex'"):
        cwt.ridge((10.0, 100.0))
    cwt._device_result, cwt._pending = ShardedResult([], (4, 3, 100), True), ("complex", np.float32, False)
    with pytest.raises(ValueError, match="sharded"):
        cwt.ridge((10.0, 100.0))
    cwt._device_result = engine.DeviceResult(None, (1, 3, 100), 128, True)
    with pytest.raises(ValueError, match="freed"):
        cwt.ridge((10.0, 100.0))
    cwt._device_result = engine.DeviceResult(object(), (1, 3, 100), 128, True)
    with pytest.raises(ValueError, match=r"bands\[1\]"):
        cwt.ridge([(10.0, 100.0), (200.0, 300.0)])
    with pytest.raises(ValueError, match="outputs"):
        cwt.ridge((10.0, 100.0), outputs=("phase",))
    cwt._device_result = None


# -- the C entry point: arguments first, then the device ----------------------------------------------------------------
def test_entry_point_validates_then_needs_a_device():
    from ghost_amd import _lib
    from ghost_amd.engine import device_count
    lib = _lib.lib
    buf = (C.c_float * 256)()
    good = (C.c_int32 * 4)(0, 4, 1, 2)
    pos = (C.c_float * 4)(1.0, 2.0, 0.5, 3.0)
    adv = (C.c_float * 4)(0.0, 2.0, 0.5, 9.0)
    two = (C.c_int64 * 4)(0, 7, 7, 16)

    def call(rows=buf, pitch=16, c=1, s=4, n=16, bands=good, n_b=2, e=pos, nu=adv, hz=1000.0, seg=two, n_seg=2, row=buf, amp=buf,
             off=buf, frq=buf, out_pitch=16):
        return lib.gcwt_ridge(rows, pitch, c, s, n, bands, n_b, e, nu, hz, seg, n_seg, row, amp, off, frq, out_pitch)

    def f4(*v):
        return (C.c_float * 4)(*v)

    def s4(*v):
        return (C.c_int64 * 4)(*v)

    for kw, word in ((dict(rows=None), b"d_rows is NULL"), (dict(bands=None), b"bands is NULL"), (dict(e=None), b"e is NULL"),
                     (dict(nu=None), b"nu is NULL"), (dict(seg=None), b"segments"), (dict(n_seg=0), b"segments"),
                     (dict(c=0), b"n_channels"), (dict(s=0), b"n_scales"), (dict(n=0), b"n_cols"), (dict(pitch=15), b"pitch"),
                     (dict(n_b=0), b"n_bands"), (dict(bands=(C.c_int32 * 4)(0, 4, -1, 2)), b"band 1"),
                     (dict(bands=(C.c_int32 * 4)(0, 0, 1, 2)), b"band 0"), (dict(bands=(C.c_int32 * 4)(0, 4, 3, 2)), b"band 1"),
                     (dict(e=f4(1, float("nan"), 1, 1)), b"e[1]"), (dict(e=f4(1, 1, 1, float("inf"))), b"e[3]"),
                     (dict(e=f4(0, 1, 1, 1)), b"e[0]"), (dict(e=f4(1, 1, -1, 1)), b"e[2]"),
                     (dict(nu=f4(0, float("nan"), 1, 1)), b"nu[1]"), (dict(nu=f4(0, 1, -1e-30, 1)), b"nu[2]"),
                     (dict(nu=f4(0, 1, 1, float("inf"))), b"nu[3]"), (dict(hz=0.0), b"hz_per_cycle"),
                     (dict(hz=float("nan")), b"hz_per_cycle"), (dict(hz=-1.0), b"hz_per_cycle"),
                     (dict(seg=s4(0, 0, 0, 16)), b"segments[0]"), (dict(seg=s4(1, 7, 7, 16)), b"segments[0]"),
                     (dict(seg=s4(0, 7, 8, 16)), b"segments[1]"), (dict(seg=s4(0, 7, 6, 16)), b"segments[1]"),
                     (dict(seg=s4(0, 7, 7, 17)), b"segments[1]"), (dict(seg=s4(0, 7, 7, 15)), b"segments[1]"),
                     (dict(seg=s4(0, 7, 7, 5)), b"segments[1]"), (dict(n_seg=1), b"segments[0]"), (dict(n_seg=17), b"segments"),
                     (dict(out_pitch=15), b"out_pitch"), (dict(row=None, amp=None, off=None, frq=None), b"nothing"),
                     (dict(c=2**31 - 1, n=2**40, pitch=2**40, out_pitch=2**40, seg=s4(0, 7, 7, 2**40)), b"workgroups")):
        assert call(**kw) == _lib.ERR_INVALID, kw
        msg = lib.gcwt_last_error()
        assert msg.startswith(b"gcwt_ridge:") and word in msg, (kw, msg)
    # a valid request: without a GPU there is nothing that computes it; with one, host memory is not a resident result
    n_dev = device_count()
    for kw in (dict(), dict(frq=None), dict(row=None, amp=None, off=None), dict(n_b=1), dict(seg=s4(0, 16, 0, 0), n_seg=1),
               dict(n=15, seg=s4(0, 1, 1, 15)), dict(nu=f4(0, 0, 0, 0))):
        rc = call(**kw)
        if n_dev == 0:
            assert rc == _lib.ERR_NO_DEVICE and b"no CPU path" in lib.gcwt_last_error(), kw
        else:
            assert rc == _lib.ERR_INVALID and b"device memory" in lib.gcwt_last_error(), kw
