"""detect() without a GPU: the NumPy model of the runs against a plain loop, the derived bound of the statistics against
exact rational arithmetic, engine.event_filter (keep, merge, durations -- in that order), the C entries' argument checks
(they come before any device call) and the refusals of the method and the engine.  The device side:
tests/test_gpu_detect.py."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import detect_model as dm

FS = 1000.0


# -- the model ------------------------------------------------------------------------------------------------------------
def _brute_runs(v, lo):
    """One column after the other: (start, stop, peak_col, peak) of every maximal run of v > lo."""
    runs, t, n = [], 0, len(v)
    while t < n:
        if not v[t] > lo:
            t += 1
            continue
        a = t
        best, at = v[t], t
        while t < n and v[t] > lo:
            if v[t] > best:
                best, at = v[t], t
            t += 1
        runs.append((a, t, at, best))
    return runs


def test_model_runs_are_those_of_a_plain_loop():
    rng = np.random.default_rng(0)
    for case in range(200):
        c, n = int(rng.integers(1, 4)), int(rng.integers(1, 40))
        v = rng.integers(-2, 4, (c, n)).astype(np.float32)                  # few values: ties and values equal to lo
        if case % 3 == 0:
            v[rng.random((c, n)) < 0.1] = np.nan
        if case % 5 == 0:
            v[rng.random((c, n)) < 0.1] = np.inf
        lo = rng.integers(-1, 3, c).astype(np.float32)
        got = dm.model_runs(v, lo)
        want = [(i,) + r for i in range(c) for r in _brute_runs(v[i], lo[i])]
        assert got["counts"].tolist() == [sum(1 for w in want if w[0] == i) for i in range(c)]
        assert len(got["trace"]) == len(want)
        for k, w in enumerate(want):
            assert (got["trace"][k], got["start"][k], got["stop"][k], got["peak_col"][k]) == w[:4], (case, k)
            assert got["peak"][k] == w[4] and got["peak"].dtype == np.float32
    one = dm.model_runs(np.array([0, 2, 2, 0, 3, 1, 3, 0, np.nan, 5], np.float32), 0.0)
    assert one["start"].tolist() == [1, 4, 9] and one["stop"].tolist() == [3, 7, 10] and one["peak_col"].tolist() == [1, 4, 9]
    assert dm.model_runs(np.ones((1, 7), np.float32), 1.0)["counts"].tolist() == [0]     # equal to lo is not above


def test_stats_bound_holds_for_sums_in_any_order():
    """The bound is derived for every order of summation: float64 sums front to back, back to front, pairwise and sorted
    stay inside it around the correctly rounded model, and the model sits on the exact rational value."""
    rng = np.random.default_rng(1)
    for n, offset in ((1, 0.0), (2, 0.0), (7, 3.0), (1000, 0.0), (1000, 1e4), (4097, -50.0), (3000, 1e7)):
        v = (rng.standard_normal(n) + offset).astype(np.float32)
        v[rng.random(n) < 0.2] = 0
        if not np.any(v):
            v[0] = 1
        cnt, mean, sd = dm.model_stats(v)
        nz = [Fraction(float(x)) for x in v if x != 0]
        assert cnt == len(nz)
        exact_mean = sum(nz) / cnt
        exact_var = sum(x * x for x in nz) / cnt - exact_mean ** 2
        bm, bs = dm.stats_bound(v)
        assert abs(Fraction(mean) - exact_mean) <= Fraction(bm) and bm <= 1e-12 * max(abs(mean), 1e-3) * n
        assert abs(sd - float(exact_var) ** 0.5) <= bs
        w = v.astype(np.float64)
        for order in (w, w[::-1], np.sort(w), w[np.argsort(-np.abs(w))]):
            for total in (lambda x: float(np.cumsum(x)[-1]), lambda x: float(np.sum(x))):   # a chain and NumPy's pairwise sum
                k = np.count_nonzero(order)
                m = total(order) / k
                s = max(total(order * order) / k - m * m, 0.0) ** 0.5
                assert abs(m - mean) <= bm and abs(s - sd) <= bs, (n, offset)
    assert dm.model_stats(np.zeros(9, np.float32)) == (0, 0.0, 0.0) and dm.stats_bound(np.zeros(9)) == (0.0, 0.0)
    assert dm.model_stats(np.array([0, 2, 0, 4], np.float32)) == (2, 3.0, 1.0)


# -- event_filter ---------------------------------------------------------------------------------------------------------
def _runs(rows):
    """(trace, start, stop, peak_col, peak) tuples -> the arrays trace_runs returns."""
    a = np.array(rows, dtype=np.float64).reshape(-1, 5)
    return {"trace": a[:, 0].astype(np.int64), "start": a[:, 1].astype(np.int64), "stop": a[:, 2].astype(np.int64),
            "peak_col": a[:, 3].astype(np.int64), "peak": a[:, 4].astype(np.float32)}


def _filter(runs, hi, time=None, min_gap=0.0, min_duration=0.0, max_duration=None, period=1 / FS):
    from ghost_amd.engine import event_filter
    got = event_filter(runs["trace"], runs["start"], runs["stop"], runs["peak_col"], runs["peak"], hi, time, min_gap, min_duration,
                       max_duration, period)
    want = dm.model_events(runs, np.atleast_1d(hi), time, min_gap, min_duration, max_duration, period)
    assert set(got) == {"trace", "start", "stop", "peak_col", "peak"}
    for k in want:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    return [tuple(int(got[k][i]) for k in ("trace", "start", "stop", "peak_col")) + (float(got["peak"][i]),) for i in range(len(got["trace"]))]


def test_event_filter_keeps_then_merges_then_measures():
    hi = np.array([5.0, 5.0], np.float32)
    # keep before merge: the run below hi between two kept ones does not bridge them (their own gap is 30 columns)
    runs = _runs([(0, 100, 110, 105, 9), (0, 115, 120, 117, 4), (0, 140, 150, 141, 7)])
    assert _filter(runs, hi, min_gap=0.02) == [(0, 100, 110, 105, 9.0), (0, 140, 150, 141, 7.0)]
    assert _filter(runs, hi, min_gap=0.032) == [(0, 100, 150, 105, 9.0)]
    # peak equal to hi is not kept
    assert _filter(_runs([(0, 1, 2, 1, 5), (0, 5, 6, 5, 5.0001)]), hi) == [(0, 5, 6, 5, float(np.float32(5.0001)))]
    # merge before the durations: two short runs make one event that is long enough; alone each is dropped
    runs = _runs([(0, 100, 110, 105, 9), (0, 112, 125, 120, 8)])
    assert _filter(runs, hi, min_duration=0.02) == []
    assert _filter(runs, hi, min_gap=0.005, min_duration=0.02) == [(0, 100, 125, 105, 9.0)]
    # ... and may make one that is too long
    assert _filter(runs, hi, min_gap=0.005, max_duration=0.02) == []
    assert _filter(runs, hi, max_duration=0.011) == [(0, 100, 110, 105, 9.0)]
    assert _filter(runs, hi, max_duration=0.014, min_duration=0.012) == [(0, 112, 125, 120, 8.0)]
    # the gap is from the last column of one to the first of the next: 111 - 109 = 2 columns, < 0.0021 s and not < 0.002 s
    runs = _runs([(0, 100, 110, 101, 6), (0, 111, 120, 115, 6)])
    assert len(_filter(runs, hi, min_gap=0.002)) == 2 and len(_filter(runs, hi, min_gap=0.0021)) == 1


def test_event_filter_merged_peak_and_chains():
    hi = np.zeros(3, np.float32)
    # a tie: the earlier peak; the larger one wherever it is; a chain of three merges into one
    runs = _runs([(1, 10, 20, 15, 7), (1, 22, 30, 25, 7), (1, 32, 40, 33, 6)])
    assert _filter(runs, hi, min_gap=0.01) == [(1, 10, 40, 15, 7.0)]
    runs = _runs([(1, 10, 20, 15, 6), (1, 22, 30, 25, 7), (1, 32, 40, 33, 7)])
    assert _filter(runs, hi, min_gap=0.01) == [(1, 10, 40, 25, 7.0)]
    # never across traces, however close the columns
    runs = _runs([(0, 10, 20, 15, 6), (1, 21, 30, 25, 7), (2, 5, 8, 6, 1)])
    assert len(_filter(runs, hi, min_gap=10.0)) == 3
    # a different hi per trace
    assert _filter(runs, np.array([6, 6, 0.5], np.float32)) == [(1, 21, 30, 25, 7.0), (2, 5, 8, 6, 1.0)]


def test_event_filter_counts_an_epoch_gap_with_its_real_length():
    # columns 0 .. 99 are the first epoch, 100 .. 199 the second, two seconds later on the clock
    time = np.concatenate([np.arange(100), 2000 + np.arange(100)]) / FS
    runs = _runs([(0, 90, 100, 95, 3), (0, 100, 110, 105, 4), (0, 112, 120, 115, 2)])
    hi = np.zeros(1, np.float32)
    assert _filter(runs, hi, None, min_gap=0.05) == [(0, 90, 120, 105, 4.0)]            # by columns all three are neighbours
    assert _filter(runs, hi, time, min_gap=0.05) == [(0, 90, 100, 95, 3.0), (0, 100, 120, 105, 4.0)]
    assert _filter(runs, hi, time, min_gap=1.9) == [(0, 90, 100, 95, 3.0), (0, 100, 120, 105, 4.0)]
    assert _filter(runs, hi, time, min_gap=1.902) == [(0, 90, 120, 105, 4.0)]
    # an output stride: a column is 4 samples
    assert _filter(runs, hi, None, min_duration=0.04, period=4 / FS) == [(0, 90, 100, 95, 3.0), (0, 100, 110, 105, 4.0)]


def test_event_filter_empty_and_single():
    from ghost_amd.engine import event_filter
    hi = np.ones(2, np.float32)
    assert _filter(_runs([]), hi, min_gap=0.1, min_duration=0.01) == []
    assert _filter(_runs([(1, 3, 9, 4, 2)]), hi, min_gap=0.1) == [(1, 3, 9, 4, 2.0)]
    assert _filter(_runs([(1, 3, 9, 4, 1)]), hi, min_gap=0.1) == []
    assert _filter(_runs([(1, 3, 9, 4, 2)]), hi, min_duration=0.0061) == []
    for kw in (dict(min_gap=-1.0), dict(min_gap=np.nan), dict(min_duration="1"), dict(max_duration=-0.5)):
        args = dict(min_gap=0.0, min_duration=0.0, max_duration=None)
        args.update(kw)
        with pytest.raises(ValueError, match=next(iter(kw))):
            event_filter([0], [1], [2], [1], [3.0], hi, None, args["min_gap"], args["min_duration"], args["max_duration"], 1e-3)
    with pytest.raises(ValueError, match="one entry per run"):
        event_filter([0, 0], [1], [2], [1], [3.0], hi, None, 0.0, 0.0, None, 1e-3)


# -- the C entries: arguments first, then the device ----------------------------------------------------------------------
def test_entry_points_validate_then_need_a_device():
    from ghost_amd import _lib
    from ghost_amd.engine import device_count
    lib = _lib.lib
    buf = (C.c_float * 256)()
    out = (C.c_int64 * 64)()
    lo = (C.c_float * 4)(0.5, 1.0, 0.0, -2.0)
    cnt = (C.c_int64 * 4)()
    dbl = (C.c_double * 4)()

    def runs(trace=buf, pitch=64, c=4, n=60, lo=lo, cap=16, start=out, stop=out, col=out, peak=buf, counts=cnt):
        return lib.gcwt_trace_runs(trace, pitch, c, n, lo, cap, start, stop, col, peak, counts)

    def stats(trace=buf, pitch=64, c=4, n=60, cnt=cnt, mean=dbl, sd=dbl):
        return lib.gcwt_trace_stats(trace, pitch, c, n, cnt, mean, sd)

    def f4(*v):
        return (C.c_float * 4)(*v)

    shared = ((dict(trace=None), b"d_trace is NULL"), (dict(c=0), b"n_traces"), (dict(c=-3), b"n_traces"), (dict(n=0), b"n_cols"),
              (dict(pitch=59), b"pitch"), (dict(n=2**40, pitch=2**40), b"n_cols"), (dict(c=2**31, n=1), b"workgroups"),
              (dict(c=2**22, n=2**39, pitch=2**39), b"workgroups"))
    for call, name, cases in ((runs, b"gcwt_trace_runs:", shared + (
            (dict(lo=None), b"lo is NULL"), (dict(counts=None), b"counts is NULL"), (dict(lo=f4(0, float("nan"), 0, 0)), b"lo[1]"),
            (dict(lo=f4(0, 0, 0, float("inf"))), b"lo[3]"), (dict(lo=f4(float("-inf"), 0, 0, 0)), b"lo[0]"), (dict(cap=-1), b"capacity"),
            (dict(start=None), b"NULL"), (dict(stop=None), b"NULL"), (dict(col=None), b"NULL"), (dict(peak=None), b"NULL"))),
                              (stats, b"gcwt_trace_stats:", shared + (
            (dict(cnt=None), b"NULL"), (dict(mean=None), b"NULL"), (dict(sd=None), b"NULL")))):
        for kw, word in cases:
            assert call(**kw) == _lib.ERR_INVALID, (name, kw)
            msg = lib.gcwt_last_error()
            assert msg.startswith(name) and word in msg, (kw, msg)
    # valid requests: without a GPU there is nothing that computes them; with one, host memory is not a trace on a device
    n_dev = device_count()
    for call, kws in ((runs, (dict(), dict(cap=0, start=None, stop=None, col=None, peak=None), dict(pitch=60), dict(c=1, n=1))),
                      (stats, (dict(), dict(pitch=60), dict(c=1, n=1)))):
        for kw in kws:
            rc = call(**kw)
            if n_dev == 0:
                assert rc == _lib.ERR_NO_DEVICE and b"no CPU path" in lib.gcwt_last_error(), kw
            else:
                assert rc == _lib.ERR_INVALID and b"device memory" in lib.gcwt_last_error(), kw


def test_engine_wrappers_refuse_before_the_library():
    from ghost_amd import engine
    with pytest.raises(ValueError, match="freed"):
        engine.trace_stats(C.c_void_p(), 64, 1, 60)
    with pytest.raises(ValueError, match="freed"):
        engine.trace_runs(None, 64, 1, 60, [0.0])
    with pytest.raises(ValueError, match="n_cols"):
        engine.trace_stats(4096, 64, 1, 60.0)
    for bad in ([0.0, 1.0], 0.0, [[0.0]], [True], ["a"]):
        with pytest.raises(ValueError, match="'lo'"):
            engine.trace_runs(4096, 64, 1, 60, bad)
    with pytest.raises(_lib_error(), match="lo\\[0\\]"):
        engine.trace_runs(4096, 64, 1, 60, [np.nan])


def _lib_error():
    from ghost_amd._lib import GhostCwtError
    return GhostCwtError


# -- detect(): refusals that need no device --------------------------------------------------------------------------------
def test_detect_before_any_transform_raises():
    from ghost_amd.wave import ContinuousWaveletTransform
    with pytest.raises(ValueError, match="transform"):
        ContinuousWaveletTransform().detect((120.0, 200.0))
    with pytest.raises(TypeError):
        ContinuousWaveletTransform().detect((120.0, 200.0), "power")                   # keywords only
    with pytest.raises(TypeError):
        ContinuousWaveletTransform().detect()


def test_detect_refuses_results_and_arguments_it_cannot_use():
    from ghost_amd import engine
    from ghost_amd.multi import ShardedResult
    from ghost_amd.wave import ContinuousWaveletTransform
    cwt = ContinuousWaveletTransform()
    cwt._frequencies, cwt._fs = np.geomspace(100.0, 10.0, 3), FS
    cwt._device_result, cwt._pending = engine.DeviceResult(object(), (1, 3, 100), 128, False), ("amplitude", np.float32, True)
    with pytest.raises(ValueError, match=r"detect\(\).*output='complex'"):
        cwt.detect((10.0, 100.0))
    cwt._device_result, cwt._pending = ShardedResult([], (4, 3, 100), True), ("complex", np.float32, False)
    with pytest.raises(ValueError, match=r"detect\(\).*sharded"):
        cwt.detect((10.0, 100.0))
    # from here on a stub whose buffer no device call could survive: every refusal comes before the first one
    cwt._device_result = engine.DeviceResult(object(), (1, 3, 100), 128, True)
    for bad in ("phase", "analytic", None, ("envelope",), 3):
        with pytest.raises(ValueError, match=r"detect\(\): 'on'"):
            cwt.detect((10.0, 100.0), on=bad)
    for bad in ("mad", "SD", None, 1.0):
        with pytest.raises(ValueError, match=r"detect\(\): 'units'"):
            cwt.detect((10.0, 100.0), units=bad)
    for units in ("sd", "absolute"):
        with pytest.raises(ValueError, match=r"detect\(\): hi < lo"):
            cwt.detect((10.0, 100.0), threshold=1.0, edge=2.0, units=units)
    with pytest.raises(ValueError, match=r"detect\(\): lo < 0"):
        cwt.detect((10.0, 100.0), threshold=1.0, edge=-0.5, units="absolute")
    with pytest.raises(ValueError, match="not finite in float32"):
        cwt.detect((10.0, 100.0), threshold=1e39, units="absolute")
    for kw in (dict(threshold=np.nan), dict(edge=np.inf), dict(threshold="3"), dict(edge=True)):
        with pytest.raises(ValueError, match="'%s' must be a finite number" % next(iter(kw))):
            cwt.detect((10.0, 100.0), **kw)
    for kw in (dict(min_gap=-1.0), dict(min_duration=np.nan), dict(max_duration=-2.0)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            cwt.detect((10.0, 100.0), **kw)
    with pytest.raises(ValueError, match=r"bands\[0\]"):
        cwt.detect((200.0, 300.0))                                                     # a band with no rows
    with pytest.raises(ValueError, match="one band"):
        cwt.detect([(10.0, 100.0), (10.0, 50.0)])
    cwt._device_result = engine.DeviceResult(None, (1, 3, 100), 128, True)
    with pytest.raises(ValueError, match="freed"):
        cwt.detect((10.0, 100.0))
    cwt._device_result = None


# -- the estimator on the oracle's coefficients: what the end-to-end test then asks of the device ---------------------------
def test_the_model_finds_the_bursts_on_the_oracles_coefficients():
    """tests/test_gpu_detect.py asks that detect() find every burst of detect_model.recording() exactly once.  That the
    definition itself does -- on the oracle's float64 coefficients, for the envelope and the power, at every column and at
    every fourth -- is settled here, so that the condition there tests the device and not the estimator."""
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
            stats = [dm.model_stats(v) for v in trace]
            mean, sd = np.array([s[1] for s in stats]), np.array([s[2] for s in stats])
            hi, lo = (mean + 3.0 * sd).astype(np.float32), mean.astype(np.float32)
            runs = dm.model_runs(trace, lo)
            ev = dm.model_events(runs, hi, t, 0.0, 0.0, None, stride / dm.FS)
            assert dm.found(ev["trace"], t[ev["peak_col"]], ev["start"], ev["stop"], ts, stride) == [], (on, stride)
            # with room to spare: the peaks are far above hi, and the lowest column between the two bursts 40 ms apart far below lo
            assert np.all(ev["peak"] > 1.3 * hi[ev["trace"]]), (on, stride)
            between = trace[1, (dm.BURSTS[1][1] + dm.BURST) // stride + 1:dm.BURSTS[1][2] // stride]
            assert between.min() < 0.7 * lo[1], (on, stride)
            merged = dm.model_events(runs, hi, t, 0.06, 0.0, None, stride / dm.FS)
            assert np.bincount(merged["trace"], minlength=2).tolist() == [4, 3], (on, stride)
