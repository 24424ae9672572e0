"""triggered() on the host side (no GPU): the event-to-column mapping, the argument checks of gcwt_triggered before any
device call, the grid it launches (include/ghostcwt_debug.h: gcwt_debug_triggered_grid), the refusals of the engine and
the class, and the float64 model of the definition (tests/triggered_model.py) on the oracle's coefficients."""
import ctypes as C

import numpy as np
import pytest

import triggered_model as tm
from oracle import ghost_oracle as orc


# -- events -> columns --------------------------------------------------------------------------------------------------
def test_columns_on_a_plain_grid():
    from ghost_amd.engine import trigger_columns
    fs, n = 1000.0, 5000
    t = 2.5 + np.arange(n) / fs
    ev = [3.0, 2.7004, 2.6996, 4.0, 3.0, 2.6, 7.399, 7.3996, 2.5994, 1.0, 9.0]
    cols, used, nb, na = trigger_columns(ev, t, fs, 1, 0.1, 0.1)
    assert (nb, na) == (100, 100) and cols.dtype == np.int64 and used.dtype == np.bool_
    # in the order given, repeats kept; column 100 and column n - 1 - 100 are the first and last whose window fits
    assert cols.tolist() == [500, 200, 200, 1500, 500, 100, 4899]
    assert used.tolist() == [True, True, True, True, True, True, True, False, False, False, False]
    cols, used, nb, na = trigger_columns(np.array([2.5, 7.499, 7.4996]), t, fs, 1, 0, 0.0)
    assert (nb, na) == (0, 0) and cols.tolist() == [0, 4999] and used.tolist() == [True, True, False]
    cols, used, nb, na = trigger_columns(np.array([3, 4], dtype=np.int32), t, fs, 1, 0.0304, 0.2496)
    assert (nb, na) == (30, 250) and cols.tolist() == [500, 1500]
    cols, used, nb, na = trigger_columns(np.array([]), t, fs, 1, 0.1, 0.1)
    assert cols.shape == (0,) and used.shape == (0,)


def test_columns_on_a_strided_grid():
    from ghost_amd.engine import trigger_columns
    fs, n, k = 1000.0, 30001, 4
    t = (3.25 + np.arange(n) / fs)[::k]                     # 7501 columns, 4 ms apart
    cols, used, nb, na = trigger_columns([3.25 + 1.0, 3.25 + 1.0019, 3.25 + 1.0021, 3.25 + 0.048, 3.25 + 29.9, 3.25 + 30.0],
                                         t, fs, k, 0.05, 0.1)
    assert (nb, na) == (12, 25)                             # round(12.5) = 12: to even, as Python rounds
    assert cols.tolist() == [250, 250, 251, 12, 7475] and used.tolist() == [True, True, True, True, True, False]
    assert t.size - 1 - na == 7475


def test_columns_with_two_epochs():
    from ghost_amd.engine import trigger_columns
    fs = 100.0
    t = np.concatenate([np.arange(300) / fs, 10.0 + np.arange(500) / fs])      # columns 0 .. 299 and 300 .. 799
    ev = [1.0,                       # inside the first epoch
          5.0,                       # in the gap
          2.9, 10.05,                # the window would cross the gap, from either side
          0.2, 14.69,                # the windows touch column 0 and the last column exactly
          0.19, 14.7,                # ... and leave by one column
          2.69, 10.2,                # the windows touch the gap's edges exactly
          3.004, 2.996, 9.9951]      # just past / before an epoch: nearest column within half a period or not
    cols, used, nb, na = trigger_columns(ev, t, fs, 1, 0.2, 0.3)
    assert (nb, na) == (20, 30)
    assert used.tolist() == [True, False, False, False, True, True, False, False, True, True, False, False, False]
    assert cols.tolist() == [100, 20, 769, 269, 320]
    # (3.004 and 2.996 lie more than half a column period from column 299; 9.9951 is within one of column 300, whose
    # window would cross)
    from ghost_amd.engine import _trigger_scan
    why = _trigger_scan(ev, t, fs, 1, 0.2, 0.3, None)[4]
    assert why == {"gap": 3, "edge": 2, "splice": 3}
    # with no window every column of either epoch can be used, and only the gap drops
    cols, used, _, _ = trigger_columns(ev, t, fs, 1, 0, 0)
    assert used.tolist() == [True, False] + [True] * 8 + [False, False, True]
    assert cols[[1, 2]].tolist() == [290, 305]


def test_columns_without_timestamps():
    from ghost_amd.engine import trigger_columns
    cols, used, nb, na = trigger_columns([0.0, 0.01, 1.0, 4.98, 4.99, -0.5], None, 100.0, 1, 0.01, 0.01, n_cols=500)
    assert (nb, na) == (1, 1) and cols.tolist() == [1, 100, 498] and used.tolist() == [False, True, True, True, False, False]
    cols, used, nb, na = trigger_columns([1.0, 1.03], None, 100.0, 2, 0.1, 0.0)          # columns are 20 ms apart
    assert (nb, na) == (5, 0) and cols.tolist() == [50, 52]


@pytest.mark.parametrize("events", [[[1.0, 2.0]], 1.0, None, ["1.0"], [1.0, np.nan], [np.inf], [True, False], [1 + 0j]])
def test_columns_refuse_bad_events(events):
    from ghost_amd.engine import trigger_columns
    with pytest.raises(ValueError, match="events"):
        trigger_columns(events, None, 1000.0, 1, 0.1, 0.1)


@pytest.mark.parametrize("bad", [-0.1, np.nan, np.inf, None, "0.1", True, (0.1,), 1j])
def test_columns_refuse_bad_windows(bad):
    from ghost_amd.engine import trigger_columns
    with pytest.raises(ValueError, match="before"):
        trigger_columns([1.0], None, 1000.0, 1, bad, 0.1)
    with pytest.raises(ValueError, match="after"):
        trigger_columns([1.0], None, 1000.0, 1, 0.1, bad)


# -- the class and the engine: refusals that need no device --------------------------------------------------------------
def test_triggered_before_any_transform_raises():
    from ghost_amd.wave import ContinuousWaveletTransform
    with pytest.raises(ValueError, match="transform"):
        ContinuousWaveletTransform().triggered([1.0], before=0.1, after=0.1)
    with pytest.raises(TypeError):
        ContinuousWaveletTransform().triggered([1.0], 0.1, 0.1)                         # keywords only
    with pytest.raises(TypeError):
        ContinuousWaveletTransform().triggered([1.0], before=0.1)                       # both are required
    with pytest.raises(TypeError):
        ContinuousWaveletTransform().triggered(before=0.1, after=0.1)


def test_engine_triggered_refuses_what_is_not_a_complex_device_result():
    from ghost_amd import engine
    from ghost_amd.multi import ShardedResult
    cols = np.array([50, 60])
    with pytest.raises(ValueError, match="one device"):
        engine.triggered(ShardedResult([], (4, 3, 100), True), cols, 5, 5)
    with pytest.raises(ValueError, match="complex"):
        engine.triggered(engine.DeviceResult(object(), (4, 3, 100), 128, False), cols, 5, 5)
    with pytest.raises(ValueError, match="freed"):
        engine.triggered(engine.DeviceResult(None, (4, 3, 100), 128, True), cols, 5, 5)
    stub = engine.DeviceResult(object(), (4, 3, 100), 128, True)
    for rows in ((0, 0), (-1, 2), (2, 2), (0, 4), (0.0, 1), (True, 1), (0,)):
        with pytest.raises(ValueError, match="rows"):
            engine.triggered(stub, cols, 5, 5, rows)
    for bad in (-1, 0.5, True, None):
        with pytest.raises(ValueError, match="nb"):
            engine.triggered(stub, cols, bad, 5)
        with pytest.raises(ValueError, match="na"):
            engine.triggered(stub, cols, 5, bad)
    for bad in ([], [[50]], [50.0], [True], 50):
        with pytest.raises(ValueError, match="cols"):
            engine.triggered(stub, np.array(bad), 5, 5)
    with pytest.raises(ValueError, match="longer"):
        engine.triggered(stub, cols, 50, 50)
    with pytest.raises(ValueError, match=r"cols\[1\]"):
        engine.triggered(stub, np.array([50, 4, 3]), 5, 5)
    with pytest.raises(ValueError, match=r"cols\[0\]"):
        engine.triggered(stub, np.array([95]), 5, 5)


# -- the C entry point: arguments first, then the device ----------------------------------------------------------------
def test_entry_point_validates_then_needs_a_device():
    from ghost_amd import _lib
    from ghost_amd.engine import device_count
    lib = _lib.lib
    buf = (C.c_float * 64)()
    good = (C.c_int64 * 3)(5, 2, 12)

    def call(rows=buf, pitch=16, c=1, s=4, n=16, r0=1, n_r=2, ev=good, n_ev=3, nb=2, na=3, amp=buf, pw=buf, evk=buf, vec=buf,
             itpc=buf, out_pitch=6):
        return lib.gcwt_triggered(rows, pitch, c, s, n, r0, n_r, ev, n_ev, nb, na, amp, pw, evk, vec, itpc, out_pitch)

    for kw, word in ((dict(rows=None), b"NULL"), (dict(ev=None), b"events"), (dict(c=0), b"n_channels"), (dict(s=0), b"n_scales"),
                     (dict(n=0), b"n_cols"), (dict(pitch=15), b"pitch"), (dict(r0=-1), b"rows"), (dict(n_r=0), b"rows"),
                     (dict(r0=3, n_r=2), b"rows"), (dict(r0=4, n_r=1), b"rows"), (dict(r0=2**31 - 1, n_r=2**31 - 1), b"rows"),
                     (dict(n_ev=0), b"n_events"), (dict(n_ev=-3), b"n_events"), (dict(n_ev=2**24 + 1), b"n_events"),
                     (dict(nb=-1), b"before"), (dict(na=-1), b"after"), (dict(nb=8, na=8), b"n_cols"),
                     (dict(nb=2**62, na=2**62), b"n_cols"), (dict(nb=2**63 - 1, na=2**63 - 1), b"n_cols"),
                     (dict(ev=(C.c_int64 * 3)(5, 1, 12)), b"event 1"), (dict(ev=(C.c_int64 * 3)(5, 2, 13)), b"event 2"),
                     (dict(ev=(C.c_int64 * 3)(-1, 1, 13)), b"event 0"), (dict(ev=(C.c_int64 * 3)(5, 2, 2**62)), b"event 2"),
                     (dict(out_pitch=5), b"out_pitch"),
                     (dict(amp=None, pw=None, evk=None, vec=None, itpc=None), b"nothing")):
        assert call(**kw) == _lib.ERR_INVALID, kw
        msg = lib.gcwt_last_error()
        assert b"gcwt_triggered" in msg and word in msg, (kw, msg)
    # a valid request (the edge events; the whole recording as one window; four outputs left out): without a GPU there is
    # nothing that computes it; with one, host memory is not a resident result
    n_dev = device_count()
    for kw in (dict(), dict(nb=0, na=0, ev=(C.c_int64 * 3)(0, 15, 0)), dict(nb=7, na=8, ev=(C.c_int64 * 1)(7), n_ev=1, out_pitch=16),
               dict(amp=None, pw=None, evk=None, vec=None), dict(n_r=3)):
        rc = call(**kw)
        if n_dev == 0:
            assert rc == _lib.ERR_NO_DEVICE and b"no CPU path" in lib.gcwt_last_error()
        else:
            assert rc == _lib.ERR_INVALID and b"device memory" in lib.gcwt_last_error()


# -- the grid ------------------------------------------------------------------------------------------------------------
def _grid(c, n_rows, nb, na):
    from ghost_amd import _lib
    rt = C.c_int32()
    lt, blocks = C.c_int64(), C.c_int64()
    rc = _lib.lib.gcwt_debug_triggered_grid(c, n_rows, nb, na, C.byref(rt), C.byref(lt), C.byref(blocks))
    assert rc == 0, _lib.lib.gcwt_last_error()
    return rt.value, lt.value, blocks.value


def test_grid_covers_every_tile_of_every_channel():
    from ghost_amd import _lib
    for c, n_rows, nb, na in ((1, 1, 0, 0), (1, 4, 0, 63), (1, 5, 0, 64), (3, 14, 31, 32), (3, 14, 100, 163), (16, 40, 300, 700),
                              (128, 23, 500, 500), (2, 23, 200, 400), (9, 8, 63, 0), (5, 3, 0, 300)):
        rt, lt, blocks = _grid(c, n_rows, nb, na)
        assert (rt, lt) == (-(-n_rows // 4), -(-(nb + na + 1) // 64))            # tiles of 4 rows x 64 lags
        assert blocks == -(-(c * lt) // 8) * 8 * rt and blocks < 2 ** 31         # row tiles of a unit lie 8 workgroups apart
    assert _grid(1, 4, 0, 63) == (1, 1, 8)                                       # whole tiles
    assert _grid(1, 5, 0, 64) == (2, 2, 16)                                      # ragged in rows and in lags
    assert _grid(128, 23, 500, 500) == (6, 16, 128 * 16 * 6)
    lib = _lib.lib
    assert lib.gcwt_debug_triggered_grid(1, 4, 0, 63, None, None, None) == 0
    for c, n_rows, nb, na in ((0, 4, 0, 0), (1, 0, 0, 0), (1, 4, -1, 0), (1, 4, 0, -1), (1, 4, 2**63 - 1, 2**63 - 1),
                              (2**20, 2**20, 0, 2**20)):                         # ... and a grid that does not fit
        assert lib.gcwt_debug_triggered_grid(c, n_rows, nb, na, None, None, None) == _lib.ERR_INVALID, (c, n_rows, nb, na)


# -- the model ---------------------------------------------------------------------------------------------------------------
def test_bounds_are_the_derived_ones():
    u = 2.0 ** -24
    for e, n in ((1, 1), (2, 1), (4, 1), (5, 2), (67, 17), (500, 125), (1000, 250)):
        assert tm.chain(e) == n
        assert tm.amplitude_bound(e) == (2 + n + 2 + 1) * u
        assert tm.power_bound(e) == (2 + n + 2 + 1) * u
        assert tm.evoked_bound(e) == np.sqrt(2.0) * (n + 2 + 1) * u
        assert tm.vector_bound(e) == np.sqrt(2.0) * (4 + n + 2 + 1) * u
        assert tm.itpc_bound(e) == tm.vector_bound(e) + 3 * u


def test_model_sums_are_the_definition():
    rng = np.random.default_rng(3)
    w = rng.standard_normal((2, 5, 40)) + 1j * rng.standard_normal((2, 5, 40))
    w[1, :, 10:20] = 0
    cols = np.array([30, 5, 12, 30, 37])
    m = tm.model(w, cols, 3, 2, (1, 3))
    for name in ("amplitude", "power", "itpc", "evoked", "vector"):
        assert m[name].shape == (2, 3, 6), name
    seg = np.stack([w[0, 2, e - 3 + 4] for e in cols])                          # row 2 = the second asked for, lag index 4
    np.testing.assert_allclose(m["amplitude"][0, 1, 4], np.abs(seg).mean(), rtol=1e-14)
    np.testing.assert_allclose(m["power"][0, 1, 4], (np.abs(seg) ** 2).mean(), rtol=1e-14)
    np.testing.assert_allclose(m["evoked"][0, 1, 4], seg.mean(), rtol=1e-13)
    np.testing.assert_allclose(m["vector"][0, 1, 4], np.exp(1j * np.angle(seg)).mean(), rtol=1e-13)
    np.testing.assert_allclose(m["itpc"][0, 1, 4], abs(np.exp(1j * np.angle(seg)).mean()), rtol=1e-13)
    # zero columns add zeros: event 12's whole window lies in channel 1's zeros -- 4 of 5 events have a direction
    only = tm.model(w, np.array([12]), 2, 2)
    assert not np.any(only["amplitude"][1]) and not np.any(only["itpc"][1]) and not np.any(only["vector"][1])
    assert np.all(m["itpc"] >= 0) and np.all(m["itpc"] <= 1)
    assert np.all(m["itpc"][1] <= 0.8 + 1e-12)
    # one event: every phasor alone, itpc exactly 1 where there is signal; a constant phase: 1 and that phase
    one = tm.model(w[:1], np.array([20]), 5, 5)
    np.testing.assert_allclose(one["itpc"], 1.0, rtol=1e-12)
    same = tm.model(np.abs(w) * np.exp(0.3j), np.array([22, 30, 25]), 1, 1)
    np.testing.assert_allclose(same["itpc"], 1.0, rtol=1e-12)
    np.testing.assert_allclose(np.angle(same["vector"]), 0.3, rtol=1e-12)
    np.testing.assert_allclose(np.abs(same["evoked"]), same["amplitude"], rtol=1e-12)
    # the same absolute lag inside another (nb, na) is the same cell
    a, b = tm.model(w, cols, 3, 2), tm.model(w, cols, 1, 2)
    np.testing.assert_array_equal(a["vector"][..., 2:], b["vector"])
    g = tm.gate_bound(w[:1], cols, 3, 2, (1, 3))
    assert all(g[k].shape == (1, 3, 6) for k in g) and np.all(g["vector"] <= 2.0)
    np.testing.assert_allclose(g["amplitude"][0, 1], 1e-5 * np.abs(w[0, 2]).max(), rtol=1e-14)


def test_model_on_the_oracle_finds_the_evoked_and_the_induced_response():
    from ghost_amd.engine import trigger_columns
    n, fs = 32768, 1000.0
    x, events = tm.evoked_input(n, fs)
    assert x.shape == (2, n) and events.shape == (60,) and events[0] == 0.7
    assert np.all(np.diff(events) >= 0.399) and np.all(np.diff(events) <= 0.501) and events[-1] <= (n - 1) / fs - 0.7
    f = orc.frequency_grid(fs, n, freq_limits=(4, 200), voices_per_octave=4)
    assert f.size == 23
    w = np.stack([orc.cwt_complex(x[c], fs, f) for c in range(2)])
    cols, used, nb, na = trigger_columns(events, np.arange(n) / fs, fs, 1, 0.2, 0.4)
    assert used.all() and (nb, na) == (200, 400)
    np.testing.assert_array_equal(cols, np.round(events * fs).astype(np.int64))
    m = tm.model(w, cols, nb, na)
    tm.check_physics(m, f, nb, fs)
    gate = tm.gate_bound(w, cols, nb, na)
    print("largest gate bounds: " + ", ".join("%s %.3g" % (k, v.max()) for k, v in gate.items()))
    assert max(v.max() for v in gate.values()) <= 1e-2
