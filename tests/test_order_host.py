"""gcwt_trace_order and detect(stats='median', baseline=...) without a GPU: the NumPy model of the order statistics against
NumPy's own sort and median, the C entry's argument checks (they come before any device call), the refusals of the engine
and of detect(), and the robust estimator on the oracle's coefficients.  The device side: tests/test_gpu_order.py."""
import ctypes as C

import numpy as np
import pytest

import detect_model as dm
import order_model as om

FS = 1000.0


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# -- the model ------------------------------------------------------------------------------------------------------------
def test_ord_is_the_total_order_of_the_bit_patterns():
    f = np.array([0xffc00001, 0xffc00000, 0xff800000, 0xc0000000, 0x80000001, 0x80000000, 0x00000000, 0x00000001, 0x00800000,
                  0x3f800000, 0x7f7fffff, 0x7f800000, 0x7fc00000, 0x7fc00001], np.uint32).view(np.float32)
    o = om.ord(f)
    assert o.dtype == np.uint32 and np.all(np.diff(o.astype(np.int64)) > 0)           # -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN
    rng = np.random.default_rng(0)
    v = rng.standard_normal(1000).astype(np.float32)
    assert np.array_equal(np.argsort(om.ord(v), kind="stable"), np.argsort(v, kind="stable"))


def test_model_order_is_numpys_sort_on_finite_data():
    rng = np.random.default_rng(1)
    for n in (1, 2, 7, 64, 1000, 1001):
        v = (rng.standard_normal((3, n)) * 10.0 ** rng.integers(-3, 4, (3, 1))).astype(np.float32)
        v[1, rng.random(n) < 0.3] = 0                                       # zeros of both signs are excluded
        v[1, rng.random(n) < 0.1] = -0.0
        ranks = np.array([0, n // 3, n // 2, n - 1])
        cnt, got = om.model_order(v, ranks)
        for i in range(3):
            s = np.sort(v[i][v[i] != 0])
            assert cnt[i] == s.size
            for j, r in enumerate(ranks):
                if r < s.size:
                    assert _bits(got[i, j]) == _bits(s[r])
                else:
                    assert _bits(got[i, j]) == 0x7fc00000
    cnt, got = om.model_order(np.zeros((1, 5), np.float32), [0, 3])
    assert cnt.tolist() == [0] and _bits(got).tolist() == [[0x7fc00000] * 2]
    # a NaN is included and sorts by its sign: -NaN first, +NaN last; per-trace ranks
    v = np.array([[1.0, np.nan, -np.inf, 0.0, -np.nan, np.inf, -2.0]], np.float32)
    v[0, 4] = np.array([0xffc00000], np.uint32).view(np.float32)[0]
    cnt, got = om.model_order(v, [[0, 1, 4, 5]])
    assert cnt.tolist() == [6] and _bits(got).tolist() == [[0xffc00000, 0xff800000, 0x7f800000, 0x7fc00000]]


def test_model_median_is_numpys_on_the_float64_copy():
    rng = np.random.default_rng(2)
    for n in (1, 2, 3, 10, 11, 1000, 1001, 70 * 1024 + 3):
        v = (rng.standard_normal((2, n)) + 3.0).astype(np.float32)
        cnt, med, mad = om.model_median_mad(v)
        assert cnt.tolist() == [n, n]
        for i in range(2):
            w = v[i].astype(np.float64)
            assert med[i] == np.median(w)
            d = np.abs(v[i] - np.float32(med[i]))                           # the prescribed float32 deviations ...
            assert d.dtype == np.float32 and mad[i] == np.median(d.astype(np.float64))
    assert [a.tolist() for a in om.model_median_mad(np.zeros((1, 9), np.float32))] == [[0], [0.0], [0.0]]
    assert [a.tolist() for a in om.model_median_mad(np.array([[0, 1, 0, 2, 4, 0]], np.float32))] == [[3], [2.0], [1.0]]
    assert [a.tolist() for a in om.model_median_mad(np.array([[1, 3, 0, 2, 4, 0]], np.float32))] == [[4], [2.5], [1.0]]


def test_centred_keys_are_numpys_float32_differences():
    rng = np.random.default_rng(3)
    v = rng.standard_normal(500).astype(np.float32)
    v[:4] = [1e-40, -1e-40, 0.25, 0.25 + 2.0 ** -24]
    for c in (np.float32(0.25), np.float32(1e4), np.float32(1e-40), np.float32(-3e-39), np.float32(1.0) + np.float32(2.0 ** -23)):
        k = om.keys(v, c)
        want = np.abs(v - c)
        assert want.dtype == np.float32 and k.tobytes() == want.tobytes()
        assert np.all(np.signbit(k) == 0)
    # inclusion is decided on v: a column equal to the centre stays, with key +0; a zero column does not, whatever its key
    k = om.keys(np.array([0.25, 0.0, -0.0, 0.5], np.float32), np.float32(0.25))
    assert _bits(k).tolist() == [0, _bits(np.float32(0.25))]
    # subnormal differences are kept, not flushed
    k = om.keys(np.array([1e-40, 3e-40], np.float32), np.float32(2e-40))
    assert np.all(k > 0) and np.all(k < np.finfo(np.float32).tiny)
    cnt, got = om.model_order(np.array([[0.25, 0.0, 0.5, 1.0]], np.float32), [0, 1, 2, 3], [0.25])
    assert cnt.tolist() == [3] and _bits(got).tolist() == [[0, _bits(np.float32(0.25)), _bits(np.float32(0.75)), 0x7fc00000]]


# -- the C entry: arguments first, then the device -------------------------------------------------------------------------
def test_entry_point_validates_then_needs_a_device():
    from ghost_amd import _lib
    from ghost_amd.engine import device_count
    lib = _lib.lib
    buf = (C.c_float * 256)()
    cnt = (C.c_int64 * 4)()
    vals = (C.c_float * 16)()

    def i8(*v):
        return (C.c_int64 * 8)(*v)

    def f4(*v):
        return (C.c_float * 4)(*v)

    def order(trace=buf, pitch=64, c=4, n=60, center=None, ranks=i8(0, 1, 2, 3, 4, 5, 6, 70), n_ranks=2, cnt=cnt, out=vals):
        return lib.gcwt_trace_order(trace, pitch, c, n, center, ranks, n_ranks, cnt, out)

    cases = ((dict(trace=None), b"d_trace is NULL"), (dict(c=0), b"n_traces"), (dict(c=-3), b"n_traces"), (dict(n=0), b"n_cols"),
             (dict(pitch=59), b"pitch"), (dict(n=2**40, pitch=2**40), b"n_cols"), (dict(c=2**31, n=1), b"workgroups"),
             (dict(c=2**22, n=2**39, pitch=2**39), b"workgroups"),
             (dict(ranks=None), b"NULL"), (dict(cnt=None), b"NULL"), (dict(out=None), b"NULL"),
             (dict(n_ranks=0), b"n_ranks"), (dict(n_ranks=5), b"n_ranks"), (dict(n_ranks=-1), b"n_ranks"),
             (dict(ranks=i8(0, 1, 2, 3, 4, -1, 6, -7)), b"ranks[5]"), (dict(ranks=i8(-2**40, 0, 0, 0, 0, 0, 0, 0)), b"ranks[0]"),
             (dict(ranks=i8(0, 0, 0, -1, 0, 0, 0, 0), n_ranks=1), b"ranks[3]"),
             (dict(center=f4(0, 1, float("nan"), float("inf"))), b"center[2]"), (dict(center=f4(float("-inf"), 0, 0, 0)), b"center[0]"),
             (dict(center=f4(0, 0, 0, float("inf"))), b"center[3]"))
    for kw, word in cases:
        assert order(**kw) == _lib.ERR_INVALID, kw
        msg = lib.gcwt_last_error()
        assert msg.startswith(b"gcwt_trace_order:") and word in msg, (kw, msg)
    n_dev = device_count()
    for kw in (dict(), dict(pitch=60), dict(c=1, n=1, n_ranks=1), dict(n_ranks=1), dict(c=2, n_ranks=4), dict(center=f4(0.5, -1.0, 0.0, 1e30)),
               dict(ranks=i8(*[2**39] * 8))):
        rc = order(**kw)
        if n_dev == 0:
            assert rc == _lib.ERR_NO_DEVICE and b"no CPU path" in lib.gcwt_last_error(), kw
        else:
            assert rc == _lib.ERR_INVALID and b"device memory" in lib.gcwt_last_error(), kw


def test_engine_wrappers_refuse_before_the_library():
    from ghost_amd import engine
    from ghost_amd._lib import GhostCwtError
    with pytest.raises(ValueError, match="freed"):
        engine.trace_order(C.c_void_p(), 64, 1, 60, [0])
    with pytest.raises(ValueError, match="freed"):
        engine.trace_median_mad(None, 64, 1, 60)
    with pytest.raises(ValueError, match="n_cols"):
        engine.trace_order(4096, 64, 1, 60.0, [0])
    with pytest.raises(ValueError, match="pitch"):
        engine.trace_median_mad(4096, True, 1, 60)
    for bad in (0, [], [0, 1, 2, 3, 4], [[0], [1]], [[[0]]], [0.0], [True], ["a"], np.zeros((3, 2), np.int64)):
        with pytest.raises(ValueError, match="'ranks' must hold"):
            engine.trace_order(4096, 64, 1, 60, bad)
    with pytest.raises(ValueError, match="'ranks' must be at least 0"):
        engine.trace_order(4096, 64, 2, 60, [[0, 1], [3, -1]])
    for bad in (0.5, [0.5, 1.0], [[0.5]], [True], ["a"]):
        with pytest.raises(ValueError, match="'center' must hold"):
            engine.trace_order(4096, 64, 1, 60, [0], bad)
    for bad in ([np.nan], [np.inf], [1e39]):
        with pytest.raises(ValueError, match="'center' must be finite"):
            engine.trace_order(4096, 64, 1, 60, [0], bad)
    with pytest.raises(GhostCwtError, match="gcwt_trace_order: bad traces"):               # what the library itself refuses
        engine.trace_order(4096, 64, 1, 65, [0])


# -- detect(): refusals that need no device --------------------------------------------------------------------------------
def test_detect_refuses_stats_and_baselines_it_cannot_use():
    from ghost_amd import engine
    from ghost_amd.wave import ContinuousWaveletTransform
    cwt = ContinuousWaveletTransform()
    cwt._frequencies, cwt._fs = np.geomspace(100.0, 10.0, 3), FS
    cwt._pending = ("complex", np.float32, False)
    # a stub whose buffer no device call could survive: every refusal comes before the first one
    cwt._device_result = engine.DeviceResult(object(), (1, 3, 100), 128, True)
    for bad in ("mad", "Median", "robust", None, 1, ("median",)):
        with pytest.raises(ValueError, match=r"detect\(\): 'stats' must be 'mean' or 'median'"):
            cwt.detect((10.0, 100.0), stats=bad)
    # which message the earlier checks give is not changed by the new keywords
    with pytest.raises(ValueError, match=r"detect\(\): 'on'"):
        cwt.detect((10.0, 100.0), on="phase", stats="robust", baseline=(1.0, 0.0))
    with pytest.raises(ValueError, match=r"detect\(\): 'units'"):
        cwt.detect((10.0, 100.0), units="mad", stats="median")
    with pytest.raises(ValueError, match=r"detect\(\): 'units'"):
        cwt.detect((10.0, 100.0), units="mad", stats="robust")
    with pytest.raises(ValueError, match=r"detect\(\): hi < lo"):
        cwt.detect((10.0, 100.0), threshold=1.0, edge=2.0, stats="median")
    with pytest.raises(ValueError, match=r"bands\[0\]"):
        cwt.detect((200.0, 300.0), stats="median", baseline=(1.0, 0.0))
    # columns 0 .. 99 at 0 .. 0.099 s
    for bad in ((0.05, 0.05), (0.06, 0.02), (np.nan, 0.05), (0.0, np.inf), (-np.inf, 0.05), (0.2, 0.3), (-1.0, -0.5), (0.0101, 0.0109),
                0.05, (0.0,), (0.0, 0.01, 0.02), ("0", "1"), (True, 2.0), "ab"):
        for stats in ("mean", "median"):
            for units in ("sd", "absolute"):
                with pytest.raises(ValueError, match=r"^detect\(\): 'baseline'"):
                    cwt.detect((10.0, 100.0), baseline=bad, stats=stats, units=units)
    # with timestamps: two epochs two seconds apart; an interval inside the gap selects nothing
    cwt._time = np.concatenate([np.arange(50), 2050 + np.arange(50)]) / FS
    for bad in ((0.05, 2.05), (3.0, 4.0), (2.0991, 2.0999)):
        with pytest.raises(ValueError, match=r"^detect\(\): 'baseline'"):
            cwt.detect((10.0, 100.0), baseline=bad, stats="median")
    cwt._device_result = None


def test_baseline_columns():
    from ghost_amd.wave.transforms import _baseline_columns
    assert _baseline_columns((0.0, 0.1), None, 100, 1e-3) == (0, 100)
    assert _baseline_columns((0.01, 0.02), None, 100, 1e-3) == (10, 20)                  # t0 <= time < t1
    assert _baseline_columns((0.0105, 0.0205), None, 100, 1e-3) == (11, 21)
    assert _baseline_columns((-5.0, 50.0), None, 100, 4e-3) == (0, 100)
    assert _baseline_columns((0.0, 0.02), None, 100, 4e-3) == (0, 5)
    t = np.concatenate([np.arange(50), 2050 + np.arange(50)]) / FS
    assert _baseline_columns((2.05, 9.0), t, 100, 1e-3) == (50, 100)
    assert _baseline_columns((0.0, 2.05), t, 100, 1e-3) == (0, 50)
    assert _baseline_columns((0.04, 2.06), t, 100, 1e-3) == (40, 60)                     # across the gap: still one stretch of columns
    with pytest.raises(ValueError, match="not one stretch"):
        _baseline_columns((0.0, 0.5), np.array([0.0, 1.0, 0.25, 2.0]), 4, 1e-3)


# -- the estimator on the oracle's coefficients: what the end-to-end test then asks of the device ---------------------------
def test_the_robust_model_finds_the_bursts_on_the_oracles_coefficients():
    """tests/test_gpu_order.py asks that detect(stats='median', threshold=12, edge=2) find every burst of
    detect_model.recording() exactly once.  That the definition itself does -- on the oracle's float64 coefficients, for the
    envelope and the power, at every column and at every fourth, with room on either side of both thresholds -- is settled
    here, and so is why the estimator exists: the bursts raise the power trace's sd thirtyfold and leave its MAD alone."""
    import bandpass_model as bm
    from ghost_amd import engine
    from ghost_amd.wave import Morse
    from oracle import ghost_oracle as orc
    x, ts = dm.recording()
    f = 250.0 / 2 ** (np.arange(6) / 4)                                     # freq_limits=[100, 250] at 4 voices per octave
    rows = engine.band_rows(dm.BAND, f)
    assert rows.tolist() == [[2, 3]]
    g, h = engine.band_weights(f, Morse(fs=dm.FS))
    epochs = np.array([[0, dm.SPLIT], [dm.SPLIT, dm.N]])
    w = np.stack([orc.cwt_complex(x[ch], dm.FS, f, epoch_bounds=epochs) for ch in range(2)])
    ref = bm.model(w, rows, g, h)
    for on in ("envelope", "power"):
        for stride in (1, 4):
            trace, t = ref[on][:, 0, ::stride].astype(np.float32), ts[::stride]
            cnt, median, mad = om.model_median_mad(trace)
            assert cnt.tolist() == [trace.shape[1]] * 2
            spread = om.MAD_TO_SD * mad
            hi, lo = (median + 12.0 * spread).astype(np.float32), (median + 2.0 * spread).astype(np.float32)
            runs = dm.model_runs(trace, lo)
            ev = dm.model_events(runs, hi, t, 0.0, 0.0, None, stride / dm.FS)
            assert dm.found(ev["trace"], t[ev["peak_col"]], ev["start"], ev["stop"], ts, stride) == [], (on, stride)
            kept = runs["peak"] > hi[runs["trace"]]
            print(on, stride, "kept / hi >=", (runs["peak"][kept] / hi[runs["trace"]][kept]).min(),
                  "rejected / hi <=", (runs["peak"][~kept] / hi[runs["trace"]][~kept]).max())
            assert np.all(ev["peak"] > 1.5 * hi[ev["trace"]]), (on, stride)
            assert np.all(runs["peak"][~kept] < 0.8 * hi[runs["trace"]][~kept]), (on, stride)
            between = trace[1, (dm.BURSTS[1][1] + dm.BURST) // stride + 1:dm.BURSTS[1][2] // stride]
            assert between.min() < 0.6 * lo[1], (on, stride, between.min() / lo[1])
            merged = dm.model_events(runs, hi, t, 0.06, 0.0, None, stride / dm.FS)
            assert np.bincount(merged["trace"], minlength=2).tolist() == [4, 3], (on, stride)
            if on == "power":
                sd = np.array([dm.model_stats(v)[2] for v in trace])
                assert np.all(1.4826 * mad < sd / 3), (stride, mad, sd)
