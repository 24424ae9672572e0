"""coupling(surrogates=...) on the host side (no GPU): the shift list, the argument checks of gcwt_coupling_surrogates
before any device call, the grid it launches (include/ghostcwt_debug.h: gcwt_debug_coupling_surrogates_grid), and the
float64 model of the definition (tests/coupling_surrogates_model.py) on the oracle's coefficients."""
import ctypes as C

import numpy as np
import pytest

import coupling_model as pm
import coupling_surrogates_model as sm
from oracle import ghost_oracle as orc

MAX_WINDOW = 2048                                           # GCWT_COUPLING_SURROGATES_MAX_WINDOW


# -- the shift list ----------------------------------------------------------------------------------------------------
def test_shift_list_is_the_documented_draw():
    from ghost_amd.engine import surrogate_shifts
    s = surrogate_shifts(200, 2048, 228, 0)
    assert s.dtype == np.int64 and s.shape == (200,)
    assert s.min() >= 228 and s.max() <= 2048 - 228
    np.testing.assert_array_equal(s, np.random.default_rng(0).integers(228, 2048 - 228 + 1, size=200))
    np.testing.assert_array_equal(s, surrogate_shifts(200, 2048, 228, 0))
    assert np.any(s != surrogate_shifts(200, 2048, 228, 1))
    two = surrogate_shifts(np.int64(2), np.int32(3), np.int64(1), 5)                                # numpy integers pass
    assert two.shape == (2,) and set(two.tolist()) <= {1, 2}
    assert set(surrogate_shifts(4096, 3, 1, 2).tolist()) == {1, 2}                                  # the smallest window
    assert set(surrogate_shifts(64, 9, 4, 2).tolist()) <= {4, 5}


@pytest.mark.parametrize("kw", [dict(k=1), dict(k=4097), dict(k=True), dict(k=200.0), dict(k=0), dict(k=None),
                                dict(window=2 * 228), dict(window=2, min_cols=1), dict(min_cols=0), dict(min_cols=1.5),
                                dict(window=1), dict(window=2048.0)])
def test_shift_list_refusals(kw):
    from ghost_amd.engine import surrogate_shifts
    args = dict(k=200, window=2048, min_cols=228, seed=0)
    args.update(kw)
    with pytest.raises(ValueError):
        surrogate_shifts(**args)


def test_coupling_with_surrogates_before_any_transform_raises():
    from ghost_amd.wave import ContinuousWaveletTransform
    with pytest.raises(ValueError, match="transform"):
        ContinuousWaveletTransform().coupling(phase=(4, 16), amplitude=(30, 200), window=64, surrogates=20)
    with pytest.raises(TypeError):
        ContinuousWaveletTransform().coupling((4, 16), (30, 200), 64, 20)                # keywords only


def test_engine_refuses_before_any_device_call():
    from ghost_amd import engine
    from ghost_amd.multi import ShardedResult
    res = engine.DeviceResult(object(), (4, 3, 5000), 5024, True)
    ok = np.array([1, 2, 3], dtype=np.int64)
    with pytest.raises(ValueError, match="one device"):
        engine.coupling_surrogates(ShardedResult([], (4, 3, 5000), True), (0, 1), (1, 2), 64, ok)
    with pytest.raises(ValueError, match="complex"):
        engine.coupling_surrogates(engine.DeviceResult(object(), (4, 3, 5000), 5024, False), (0, 1), (1, 2), 64, ok)
    with pytest.raises(ValueError, match="window"):
        engine.coupling_surrogates(res, (0, 1), (1, 2), 1, ok)
    with pytest.raises(ValueError, match=str(MAX_WINDOW)):
        engine.coupling_surrogates(res, (0, 1), (1, 2), MAX_WINDOW + 1, ok)
    with pytest.raises(ValueError, match="phase_rows"):
        engine.coupling_surrogates(res, (0, 4), (1, 2), 64, ok)
    with pytest.raises(ValueError, match="amp_rows"):
        engine.coupling_surrogates(res, (0, 1), (3, 1), 64, ok)
    for bad in ([1], list(range(4097)), [1.0, 2.0], [True, False], [[1, 2]], [1, 64], [-1, 3]):
        with pytest.raises(ValueError, match="shifts"):
            engine.coupling_surrogates(res, (0, 1), (1, 2), 64, np.array(bad))


# -- the C entry point: arguments first, then the device ----------------------------------------------------------------
def test_entry_point_validates_then_needs_a_device():
    from ghost_amd import _lib
    from ghost_amd.engine import device_count
    lib = _lib.lib
    assert _lib.COUPLING_SURROGATES_MAX_WINDOW == MAX_WINDOW and MAX_WINDOW >= 2048
    buf = (C.c_float * 64)()

    def call(rows=buf, pitch=16, c=1, s=4, n=16, p0=2, n_p=2, a0=0, n_a=3, window=4, shifts=(1, 2, 3), k=None, mean=buf, sd=buf,
             count=buf, sur=None, out_pitch=4):
        arr = None if shifts is None else (C.c_int64 * len(shifts))(*shifts)
        return lib.gcwt_coupling_surrogates(rows, pitch, c, s, n, p0, n_p, a0, n_a, window, arr,
                                            len(shifts) if k is None else k, mean, sd, count, sur, out_pitch)

    big = dict(pitch=MAX_WINDOW + 16, n=MAX_WINDOW + 16, out_pitch=2)
    for kw, word in ((dict(rows=None), b"NULL"), (dict(shifts=None, k=3), b"NULL"), (dict(window=1), b"window"),
                     (dict(pitch=15), b"pitch"), (dict(n=0), b"n_cols"), (dict(s=0), b"n_scales"), (dict(c=0), b"n_channels"),
                     (dict(p0=-1), b"phase"), (dict(n_p=0), b"phase"), (dict(p0=3, n_p=2), b"phase"),
                     (dict(a0=-1), b"amplitude"), (dict(n_a=0), b"amplitude"), (dict(n_a=5), b"amplitude"),
                     (dict(window=MAX_WINDOW + 1, **big), b"GCWT_COUPLING_SURROGATES_MAX_WINDOW = %d" % MAX_WINDOW),
                     (dict(shifts=(1, -1, 2)), b"shift 1"), (dict(shifts=(1, 2, 4)), b"shift 2"),
                     (dict(shifts=(0, MAX_WINDOW), window=MAX_WINDOW, **big), b"shift 1"),
                     (dict(shifts=(1,)), b"n_shifts"), (dict(shifts=(1,) * 4097), b"n_shifts"), (dict(k=0), b"n_shifts"),
                     (dict(out_pitch=3), b"out_pitch"),
                     (dict(mean=None, sd=None, count=None, sur=None), b"nothing")):
        assert call(**kw) == _lib.ERR_INVALID, kw
        assert word in lib.gcwt_last_error(), (kw, lib.gcwt_last_error())
    # valid requests (the largest window, 4096 shifts, one output only): without a GPU there is nothing that computes
    # them; with one, host memory is not a resident result
    n_dev = device_count()
    for kw in (dict(), dict(window=MAX_WINDOW, shifts=(0, MAX_WINDOW - 1), **big), dict(shifts=(3,) * 4096),
               dict(mean=None, sd=None, count=None, sur=buf), dict(sd=None, count=None)):
        rc = call(**kw)
        if n_dev == 0:
            assert rc == _lib.ERR_NO_DEVICE and b"no CPU path" in lib.gcwt_last_error(), (kw, lib.gcwt_last_error())
        else:
            assert rc == _lib.ERR_INVALID and b"device memory" in lib.gcwt_last_error(), (kw, lib.gcwt_last_error())


# -- the grid ----------------------------------------------------------------------------------------------------------
def _grid(c, n, n_p, n_a, window):
    from ghost_amd import _lib
    pt, at = C.c_int32(), C.c_int32()
    nb, lds = C.c_int64(), C.c_int64()
    rc = _lib.lib.gcwt_debug_coupling_surrogates_grid(c, n, n_p, n_a, window, C.byref(pt), C.byref(at), C.byref(nb), C.byref(lds))
    assert rc == 0, _lib.lib.gcwt_last_error()
    return pt.value, at.value, nb.value, lds.value


def test_grid_covers_every_tile_of_every_channel_and_bin_and_fits_the_lds():
    from ghost_amd import _lib
    tail = None
    for c, n, n_p, n_a, window in ((1, 5003, 1, 1, 2), (3, 5003, 5, 9, 100), (128, 1000000, 8, 11, 1000), (128, 1000000, 8, 11, 2048),
                                   (16, 1 << 18, 12, 20, 1001), (9, 5003, 4, 8, 2047), (2, 70000, 13, 17, 3)):
        pt, at, blocks, lds = _grid(c, n, n_p, n_a, window)
        assert (pt, at) == (-(-n_p // 4), -(-n_a // 8))                          # tiles of 4 phase x 8 amplitude rows
        units = c * -(-n // window)                                             # one (channel, bin) each
        assert blocks == -(-units // 8) * 8 * pt * at and blocks < 2 ** 31       # tiles of a unit lie 8 workgroups apart
        cols = -(-window // 4) * 4                                              # 64 bytes per column, planes of whole 16 bytes
        tail = lds - 64 * cols if tail is None else tail
        assert lds == 64 * cols + tail and lds % 16 == 0 and lds <= 160 * 1024
    assert 0 < tail <= 16 * 1024                                                # the waves' sums
    assert _grid(128, 1000000, 8, 11, 2048)[:3] == (2, 2, 128 * 489 * 4)
    assert _grid(1, 5003, 4, 8, MAX_WINDOW)[3] == 64 * MAX_WINDOW + tail >= 128 * 1024
    lib = _lib.lib
    assert lib.gcwt_debug_coupling_surrogates_grid(1, 5003, 1, 1, MAX_WINDOW + 1, None, None, None, None) == _lib.ERR_INVALID
    assert b"MAX_WINDOW" in lib.gcwt_last_error()
    assert lib.gcwt_debug_coupling_surrogates_grid(1, 100, 1, 1, 1, None, None, None, None) == _lib.ERR_INVALID
    assert lib.gcwt_debug_coupling_surrogates_grid(1, 100, 0, 1, 4, None, None, None, None) == _lib.ERR_INVALID
    assert lib.gcwt_debug_coupling_surrogates_grid(30000, 1 << 33, 64, 64, 2, None, None, None, None) == _lib.ERR_INVALID
    assert b"workgroups" in lib.gcwt_last_error()
    assert lib.gcwt_debug_coupling_surrogates_grid(1, 100, 1, 1, 4, None, None, None, None) == 0


# -- the model ---------------------------------------------------------------------------------------------------------
def test_bounds_are_the_derived_ones():
    u, e = 2.0 ** -24, 2.0 ** -53
    for w in (2, 64, 65, 1000, 2048):
        assert sm.surrogate_bound(w) == pm.mvl_bound(w)
        for k in (2, 7, 200, 4096):
            assert sm.mean_bound(w, k) == pm.mvl_bound(w) + k * e + u
            assert sm.sd_rounding(k) == np.sqrt(e * (k * (3.0 * k + 3.0) / (k - 1.0) + 1.0)) + e + u
            assert sm.sd_bound(w, k) == np.sqrt(k / (k - 1.0)) * pm.mvl_bound(w) + sm.sd_rounding(k)
    assert sm.sd_rounding(7) < 2.1 * u and sm.sd_rounding(4096) < 1.3e-6


def test_model_is_the_definition():
    rng = np.random.default_rng(3)
    w = rng.standard_normal((2, 5, 23)) + 1j * rng.standard_normal((2, 5, 23))
    w[1, :, 10:20] = 0                                                           # bins 2 and 3 of channel 1: no signal
    shifts = [0, 1, 3, 4]
    m = sm.model(w, (1, 2), (2, 3), 5, shifts)
    assert m["mvl"].shape == (4, 2, 2, 3, 5) and m["mean"].shape == (2, 2, 3, 5) and m["count"].shape == (2, 2, 3, 5)
    plain = pm.model(w, (1, 2), (2, 3), 5)
    np.testing.assert_allclose(m["mvl"][0], plain["mvl"], rtol=1e-12, atol=1e-15)       # L = 0 is coupling()'s mvl
    np.testing.assert_allclose(m["observed"], plain["mvl"], rtol=1e-12, atol=1e-15)
    np.testing.assert_array_equal(m["s"], plain["s"])
    # one cell by hand: a full bin and the short last one (3 columns: 4 mod 3 = 1, 3 mod 3 = 0)
    for k, shift in enumerate(shifts):
        for b, cnt, m_bin in ((5, 5, 1), (20, 3, 4)):
            idx = b + (np.arange(cnt) + shift % cnt) % cnt
            u = w[0, 2, b:b + cnt] / np.abs(w[0, 2, b:b + cnt])
            want = abs(np.sum(np.abs(w[0, 4, idx]) * u)) / np.sum(np.abs(w[0, 4, b:b + cnt]))
            np.testing.assert_allclose(m["mvl"][k, 0, 1, 2, m_bin], want, rtol=1e-12)
    np.testing.assert_array_equal(m["mvl"][2, ..., 4], m["mvl"][0, ..., 4])             # ... so shift 3 is shift 0 there
    np.testing.assert_allclose(m["mean"], m["mvl"].mean(0), rtol=1e-15)
    np.testing.assert_allclose(m["sd"], m["mvl"].std(0, ddof=1), rtol=1e-15)
    assert m["count"].min() >= 1 and m["count"].max() <= 4                              # shift 0 counts itself
    assert np.all(m["count"][..., 4] >= 2)
    # no signal: 0 everywhere, every surrogate >= the observed 0, p = 1 and z = 0
    assert not np.any(m["mvl"][:, 1, :, :, 2:4]) and not np.any(m["sd"][1, :, :, 2:4])
    assert np.all(m["count"][1, :, :, 2:4] == 4)
    z, p = sm.z_and_p(m["observed"], m["mean"], m["sd"], m["count"], 4)
    assert np.all(z[1, :, :, 2:4] == 0) and np.all(p[1, :, :, 2:4] == 1.0)
    assert m["mvl"].min() >= 0 and m["mvl"].max() <= 1 + 1e-12


def test_input_is_the_documented_draw():
    x = sm.jittered_input(4096, 1000.0, seed=7)
    rng = np.random.default_rng(7)
    a = np.exp(-1 / 250)
    e = rng.standard_normal(4096) * 1.5 * np.sqrt(1 - a * a)
    d = np.zeros(4096)
    d[0] = e[0]
    for i in range(1, 4096):
        d[i] = a * d[i - 1] + e[i]
    th = 2 * np.pi * np.cumsum(8 + d) / 1000.0
    t = np.arange(4096) / 1000.0
    np.testing.assert_allclose(x[0], np.cos(th) + 0.2 * (1 + 0.8 * np.cos(th - 1)) * np.sin(2 * np.pi * 80 * t)
                               + 0.2 * rng.standard_normal(4096), rtol=0, atol=1e-12)
    np.testing.assert_allclose(x[1], np.cos(th) + 0.2 * np.sin(2 * np.pi * 80 * t) + 0.2 * rng.standard_normal(4096), rtol=0, atol=1e-12)


def test_model_on_the_oracle_tells_the_coupled_channel_from_the_uncoupled_one():
    from ghost_amd.engine import surrogate_shifts
    n, fs, window, k = 32768, 1000.0, 2048, 200
    x = sm.jittered_input(n, fs)
    f = orc.frequency_grid(fs, n, freq_limits=(4, 200), voices_per_octave=4)
    rows = [int(np.argmin(np.abs(f - 8.0))), int(np.argmin(np.abs(f - 80.0)))]
    w = np.stack([np.stack([orc.cwt_complex(x[ch], fs, f[r:r + 1])[0] for r in rows]) for ch in range(2)])
    for seed in (0, 1):
        shifts = surrogate_shifts(k, window, 228, seed)
        m = sm.model(w, (0, 1), (1, 1), window, shifts)
        z, p = sm.z_and_p(m["observed"], m["mean"], m["sd"], m["count"], k)
        z, p = z[:, 0, 0], p[:, 0, 0]
        print("seed %d: channel 0 median z %.2f, largest p %.4f; channel 1 median z %.2f, median p %.3f"
              % (seed, np.median(z[0]), p[0].max(), np.median(z[1]), np.median(p[1])))
        assert np.median(z[0]) >= 3 and np.all(p[0] <= 0.02)
        assert abs(np.median(z[1])) <= 0.6 and np.median(p[1]) >= 0.25
