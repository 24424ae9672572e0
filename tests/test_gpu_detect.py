"""detect() on the MI355X (csrc/detect_runs.hip, include/ghostcwt.h: gcwt_trace_stats, gcwt_trace_runs): the runs of
uploaded traces bit for bit against the NumPy model (tests/detect_model.py) at every size and placement where the tiling,
the halo, the ranks or the peak search could go wrong; the statistics against correctly rounded sums within the bound the
model derives for any order of summation; detect() end to end, exactly against the model applied to bandpass()'s own trace
and physically on a recording whose bursts the model is known to find (tests/test_detect_host.py); its side effects."""
import ctypes as C

import numpy as np
import pytest

import detect_model as dm

pytestmark = pytest.mark.gpu

T = 1024                                            # GCWT_RUNS_TILE_COLS
SIZES = (1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T, 3 * T + 1)
FIELDS = (("start", np.int64), ("stop", np.int64), ("peak_col", np.int64), ("peak", np.float32))


def _pitch(n):
    from ghost_amd.engine import _pitch
    return _pitch(n)


def _upload(traces, pitch):
    """(C, n) float32 traces on the device, pitch elements apart; what lies between n and pitch is +inf: read perhaps, never
    a run and never counted."""
    from ghost_amd.engine import DeviceBuffer
    traces = np.asarray(traces, dtype=np.float32)
    c, n = traces.shape
    padded = np.full((c, pitch), np.inf, np.float32)
    padded[:, :n] = traces
    buf = DeviceBuffer(padded.nbytes)
    buf.upload(padded)
    return buf


def _same_runs(got, want, msg):
    assert np.array_equal(got["counts"], want["counts"]), (msg, got["counts"], want["counts"])
    for name in ("trace", "start", "stop", "peak_col", "peak"):
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, (msg, name)
        assert got[name].tobytes() == want[name].tobytes(), (msg, name, got[name][:8], want[name][:8])


def _runs_on_device(traces, lo, pitch=None):
    from ghost_amd import engine
    c, n = traces.shape
    pitch = _pitch(n) if pitch is None else pitch
    buf = _upload(traces, pitch)
    try:
        return engine.trace_runs(buf.ptr, pitch, c, n, lo)
    finally:
        buf.free()


def _placements(n, rng):
    """Traces of n columns and their thresholds: every placement of runs that the tiling, the halo and the ranks must get
    right, as far as n has room for it."""
    rows, los = [], []

    def add(v, lo):
        rows.append(np.asarray(v, dtype=np.float32)), los.append(lo)

    noise = rng.standard_normal(n)
    noise[0] = noise[-1] = 3.0                                              # runs that touch column 0 and the last column
    add(noise, 0.5)
    add(np.full(n, 2.0), 1.0)                                               # all above: one run
    add(np.full(n, 2.0), 2.0)                                               # equal to lo is not above: no run, between two traces with runs
    add(np.where(np.arange(n) % 2 == 0, 1.0, -1.0), 0.0)                    # alternating: ceil(n / 2) runs of one column
    add(np.where(np.arange(n) % 2 == 1, 1.0, -1.0), -0.5)                   # ... starting at column 1
    few = rng.integers(0, 3, n).astype(np.float64)                          # few values: many equal to lo, many tied peaks
    add(few, 1.0)
    add(few, -7.25)
    special = rng.standard_normal(n) + 1.0
    special[rng.random(n) < 0.05] = np.nan                                  # a NaN splits a run
    special[rng.random(n) < 0.05] = np.inf                                  # +inf is above and a peak
    special[rng.random(n) < 0.02] = -np.inf
    add(special, 0.0)
    if n > T:
        v = np.zeros(n)
        v[T - 5:T - 1] = 1                                                  # stops at T - 1 ...
        v[T:min(T + 3, n)] = 2                                              # ... beside one that starts at T
        add(v, 0.5)
        v = np.zeros(n)
        v[T - 1:T + 1] = [3, 4]                                             # starts at T - 1, stops at T + 1
        add(v, 0.5)
        v = np.zeros(n)
        v[3:T] = 1                                                          # the last column of a tile, then nothing
        add(v, 0.0)
    if n >= 2 * T:
        v = np.zeros(n)
        v[T:2 * T] = 1                                                      # exactly one whole tile
        v[T + 700] = v[T + 700 + 64] = 5
        add(v, 0.25)
    if n >= 3 * T:
        v = rng.random(n) + 1
        v[3 * T:] = 0                                                       # one run covering three whole tiles
        v[2 * T + 17] = v[5] = 9
        add(v, 0.5)
    return np.stack(rows), np.array(los, dtype=np.float32)


# -- 1. the runs, bit for bit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_runs_are_the_models_bit_for_bit(n):
    traces, lo = _placements(n, np.random.default_rng(n))
    want = dm.model_runs(traces, lo)
    assert want["counts"][1] == 1 and want["counts"][2] == 0 and want["counts"][3] == -(-n // 2) and want["counts"][0] >= 1
    got = _runs_on_device(traces, lo)
    _same_runs(got, want, "n=%d" % n)
    print("n=%d: %d traces, %d runs" % (n, len(lo), len(got["start"])))
    # an odd pitch (rows off 16 bytes: one load per column) and no padding at all
    for pitch in (n + 1 if n % 2 == 0 else n + 2, n):
        _same_runs(_runs_on_device(traces, lo, pitch), want, "n=%d pitch=%d" % (n, pitch))


def test_the_first_of_equal_peaks_wins():
    n, a = 2 * T + 100, 3                                                   # every run starts at column 3: lane l looks at 3 + l, 67 + l, ...
    cases = {"same lane, 64 apart": (a + 5, a + 5 + 64), "same lane, 128 apart": (a + 7 + 64, a + 7 + 192),
             "neighbouring lanes": (a + 10, a + 11), "a later lane first": (a + 40, a + 64 + 2), "lanes 0 and 63": (a + 63, a + 64),
             "three of them": (a + 300, a + 301, a + 364), "far apart": (a + 1, a + 2 * T), "the first column": (a, a + 64),
             "the last column": (a + 9, a + 2 * T + 49)}
    traces = np.ones((len(cases) + 1, n), np.float32)
    traces[:, :a] = 0
    traces[:, a + 2 * T + 50:] = 0
    for i, cols in enumerate(cases.values()):
        traces[i, list(cols)] = 5
    # all equal: the run's first column
    lo = np.full(len(traces), 0.5, np.float32)
    got = _runs_on_device(traces, lo)
    _same_runs(got, dm.model_runs(traces, lo), "ties")
    assert got["start"].tolist() == [a] * len(traces) and got["stop"].tolist() == [a + 2 * T + 50] * len(traces)
    assert got["peak_col"].tolist() == [min(cols) for cols in cases.values()] + [a]
    assert got["peak"].tolist() == [5.0] * len(cases) + [1.0]


def test_capacity_protocol():
    from ghost_amd import _lib
    from ghost_amd.engine import DeviceBuffer
    n = T + 65
    traces, lo = _placements(n, np.random.default_rng(3))
    want = dm.model_runs(traces, lo)
    total = int(want["counts"].sum())
    c, pitch = len(lo), _pitch(n)
    buf = _upload(traces, pitch)
    counts = np.zeros(c, np.int64)
    i64p, f32p = C.POINTER(C.c_int64), C.POINTER(C.c_float)

    def call(capacity, where):
        counts[:] = -1
        return _lib.lib.gcwt_trace_runs(buf.ptr, pitch, c, n, lo.ctypes.data_as(f32p), capacity, *where, counts.ctypes.data_as(i64p))

    assert call(0, (None,) * 4) == 0 and np.array_equal(counts, want["counts"])          # sizing: no arrays at all
    out = {name: DeviceBuffer((total + 1) * np.dtype(dtype).itemsize) for name, dtype in FIELDS}

    def fill():
        for name, dtype in FIELDS:
            out[name].upload(np.full(total + 1, 77, dtype))

    where = tuple(out[name].ptr for name, _ in FIELDS)
    fill()
    assert call(total - 1, where) == 0 and np.array_equal(counts, want["counts"])        # one short: GCWT_OK, nothing written
    for name, dtype in FIELDS:
        assert np.all(out[name].download((total + 1,), dtype) == 77), name
    for capacity in (total, total + 1):                                                  # exactly enough; more than enough
        fill()
        assert call(capacity, where) == 0 and np.array_equal(counts, want["counts"])
        for name, dtype in FIELDS:
            got = out[name].download((total + 1,), dtype)
            assert got[:total].tobytes() == want[name].tobytes() and got[total] == 77, (capacity, name)
    # no runs at all (in the traces without a +inf: the first seven) with room for some: nothing is written
    high = np.full(7, 3e38, np.float32)
    fill()
    counts[:] = -1
    assert _lib.lib.gcwt_trace_runs(buf.ptr, pitch, 7, n, high.ctypes.data_as(f32p), total, *where, counts.ctypes.data_as(i64p)) == 0
    assert not counts[:7].any() and np.all(out["start"].download((total + 1,), np.int64) == 77)
    for b in out.values():
        b.free()
    buf.free()


def test_runs_have_the_same_bits_alone_among_others_and_twice():
    from ghost_amd import engine
    n = 2 * T + 37
    traces, lo = _placements(n, np.random.default_rng(9))
    c, pitch = len(lo), _pitch(n)
    buf = _upload(traces, pitch)
    first = engine.trace_runs(buf.ptr, pitch, c, n, lo)
    _same_runs(engine.trace_runs(buf.ptr, pitch, c, n, lo), first, "second call")
    for i in range(c):
        alone = engine.trace_runs(buf.ptr.value + i * pitch * 4, pitch, 1, n, lo[i:i + 1])
        mine = first["trace"] == i
        assert alone["counts"].tolist() == [first["counts"][i]]
        for name, _ in FIELDS:
            assert alone[name].tobytes() == first[name][mine].tobytes(), (i, name)
    # the same buffer seen with fewer columns: the runs of the shorter traces
    for m in (1, T - 1, T, T + 1, 2 * T):
        _same_runs(engine.trace_runs(buf.ptr, pitch, c, m, lo), dm.model_runs(traces[:, :m], lo), "first %d columns" % m)
    buf.free()
    with pytest.raises(ValueError, match="freed"):
        engine.trace_runs(buf.ptr, pitch, c, n, lo)


# -- 2. the statistics -----------------------------------------------------------------------------------------------------
def _stat_traces(n, rng):
    rows = [rng.standard_normal(n), rng.standard_normal(n) + 1e4, np.abs(rng.standard_normal(n)) * 1e-3, np.zeros(n),
            rng.random(n) + 0.5, np.full(n, 0.1)]
    with_zeros = rng.random(n) + 0.5
    if n >= 3:
        with_zeros[n // 3:n // 3 + max(1, n // 4)] = 0                      # a gap: the statistics are those of the rest
    rows.append(with_zeros)
    rows.append(np.where(rng.random(n) < 0.5, 0.0, rng.standard_normal(n) * 100))
    return np.stack(rows).astype(np.float32)


def _check_stats(got, traces, msg):
    n, mean, sd = got
    assert n.dtype == np.int64 and mean.dtype == sd.dtype == np.float64 and n.shape == mean.shape == sd.shape == (len(traces),)
    worst = 0.0
    for i, v in enumerate(traces):
        cnt, m, s = dm.model_stats(v)
        bm, bs = dm.stats_bound(v)
        assert n[i] == cnt, (msg, i)
        if cnt == 0:
            assert mean[i] == 0 and sd[i] == 0, (msg, i)
            continue
        assert abs(mean[i] - m) <= bm and abs(sd[i] - s) <= bs, (msg, i, mean[i] - m, bm, sd[i] - s, bs)
        worst = max(worst, abs(mean[i] - m) / bm, abs(sd[i] - s) / bs)
    return worst


@pytest.mark.parametrize("n", SIZES + (70 * T + 3,))
def test_stats_meet_correctly_rounded_sums_within_the_derived_bound(n):
    from ghost_amd import engine
    traces = _stat_traces(n, np.random.default_rng(1000 + n))
    c = len(traces)
    worst = 0.0
    for pitch in (_pitch(n), n + 1 if n % 2 == 0 else n + 2, n):
        buf = _upload(traces, pitch)
        got = engine.trace_stats(buf.ptr, pitch, c, n)
        worst = max(worst, _check_stats(got, traces, "n=%d pitch=%d" % (n, pitch)))
        assert got[0][3] == 0 and got[1][3] == 0 and got[2][3] == 0                    # the all-zero trace
        # zeros excluded: the trace with a gap has the statistics of its other columns, which the model took alone
        again = engine.trace_stats(buf.ptr, pitch, c, n)
        for a, b in zip(got, again):
            assert a.tobytes() == b.tobytes(), "second call"
        for i in range(c):                                                            # (whatever the width of the loads then is)
            alone = engine.trace_stats(buf.ptr.value + i * pitch * 4, pitch, 1, n)
            for a, b in zip(got, alone):
                assert a[i:i + 1].tobytes() == b.tobytes(), ("alone", i)
        buf.free()
    print("n=%d: worst error / bound %.3g" % (n, worst))


def test_stats_of_nan_and_inf_columns_are_nan_or_inf():
    from ghost_amd import engine
    n = T + 9
    traces = np.ones((3, n), np.float32)
    traces[0, 5] = np.nan
    traces[1, T + 2] = np.inf
    buf = _upload(traces, _pitch(n))
    cnt, mean, sd = engine.trace_stats(buf.ptr, _pitch(n), 3, n)
    buf.free()
    assert cnt.tolist() == [n, n, n]
    assert np.isnan(mean[0]) and np.isnan(sd[0]) and mean[1] == np.inf and np.isnan(sd[1]) and mean[2] == 1.0 and sd[2] == 0.0


# -- 3. end to end ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def recorded():
    """The recording of detect_model.recording(), transformed once at every column and once at every fourth."""
    from ghost_amd.wave import ContinuousWaveletTransform
    x, ts = dm.recording()
    out = {"x": x, "ts": ts}
    for stride in (1, 4):
        cwt = ContinuousWaveletTransform()
        cwt.transform(x, fs=dm.FS, timestamps=ts, multichannel=True, output="complex", dtype=np.float32, output_stride=stride,
                      **dm.TRANSFORM)
        out[stride] = cwt
    yield out
    for stride in (1, 4):
        out[stride].release_device()


def _exactly_the_model(cwt, r, on, stride, ts, threshold, edge, units, min_gap=0.0, min_duration=0.0, max_duration=None):
    """detect()'s result against the definition applied on the host to bandpass()'s own trace, given the reported lo / hi."""
    from ghost_amd import engine
    trace = getattr(cwt.bandpass(dm.BAND, outputs=(on,)), on)[:, 0]
    t = ts[::stride]
    # the statistics: within the derived bound of the host's; lo / hi: those numbers, rounded once
    for ch in range(trace.shape[0]):
        cnt, m, s = dm.model_stats(trace[ch])
        bm, bs = dm.stats_bound(trace[ch])
        assert r.n_columns[ch] == cnt == trace.shape[1]
        assert abs(r.mean[ch] - m) <= bm and abs(r.sd[ch] - s) <= bs, (ch, r.mean[ch] - m, bm, r.sd[ch] - s, bs)
    assert r.lo.dtype == r.hi.dtype == np.float32
    if units == "sd":
        assert np.array_equal(r.hi, (r.mean + threshold * r.sd).astype(np.float32)) and np.array_equal(r.lo, (r.mean + edge * r.sd).astype(np.float32))
    else:
        assert np.all(r.hi == np.float32(threshold)) and np.all(r.lo == np.float32(edge))
    runs = dm.model_runs(trace, r.lo)
    assert np.array_equal(r.n_candidates, runs["counts"])
    want = engine.event_filter(runs["trace"], runs["start"], runs["stop"], runs["peak_col"], runs["peak"], r.hi, t, min_gap,
                               min_duration, max_duration, stride / dm.FS)
    loop = dm.model_events(runs, r.hi, t, min_gap, min_duration, max_duration, stride / dm.FS)
    for name, mine in (("trace", r.channel), ("start", r.start_col), ("stop", r.stop_col), ("peak_col", r.peak_col), ("peak", r.peak)):
        assert mine.dtype == want[name].dtype and mine.tobytes() == want[name].tobytes() == loop[name].tobytes(), name
    assert np.array_equal(r.start, t[r.start_col]) and np.array_equal(r.stop, t[r.stop_col - 1]) and np.array_equal(r.peak_time, t[r.peak_col])
    assert np.array_equal(r.peak, trace[r.channel, r.peak_col])
    assert r.on == on and r.band == dm.BAND and r.rows == (2, 3) and np.array_equal(r.frequencies, np.array(cwt.frequencies)[2:5])
    return len(r)


@pytest.mark.parametrize("on,stride", [("envelope", 1), ("power", 1), ("envelope", 4), ("power", 4)])
def test_detect_is_the_definition_on_bandpass_s_trace_and_finds_the_bursts(recorded, on, stride):
    cwt, ts = recorded[stride], recorded["ts"]
    r = cwt.detect(dm.BAND, on=on)
    n = _exactly_the_model(cwt, r, on, stride, ts, 3.0, 0.0, "sd")
    print("%s, stride %d: %d events of %s candidates; mean %s sd %s" % (on, stride, n, r.n_candidates, r.mean, r.sd))
    # the physical reading: every burst once, its peak inside it, nothing from one epoch into the other
    assert dm.found(r.channel, r.peak_time, r.start_col, r.stop_col, ts, stride) == []
    assert r.channel.tolist() == [0] * 4 + [1] * 4 and np.all(np.diff(r.start[r.channel == 1]) > 0)
    gap = (r.stop > ts[dm.SPLIT - 1]) & (r.start < ts[dm.SPLIT])                          # an event with a foot in either epoch
    assert not gap.any() and not np.any((r.peak_time > ts[dm.SPLIT - 1]) & (r.peak_time < ts[dm.SPLIT]))


def test_detect_variants(recorded):
    cwt, ts = recorded[1], recorded["ts"]
    # neighbours 40 ms apart merge under min_gap = 60 ms: three events in channel 1, the merged one holds both bursts
    r = cwt.detect(dm.BAND, min_gap=0.06)
    assert _exactly_the_model(cwt, r, "envelope", 1, ts, 3.0, 0.0, "sd", min_gap=0.06) == 7
    assert np.bincount(r.channel).tolist() == [4, 3]
    both = r.start_col[5], r.stop_col[5]
    assert both[0] <= dm.BURSTS[1][1] + 10 and both[1] >= dm.BURSTS[1][2] + dm.BURST - 10
    # ... but never across the two seconds between the epochs, however close the columns
    wide = cwt.detect(dm.BAND, min_gap=1.9)
    _exactly_the_model(cwt, wide, "envelope", 1, ts, 3.0, 0.0, "sd", min_gap=1.9)
    assert not np.any((wide.start_col < dm.SPLIT) & (wide.stop_col > dm.SPLIT))
    # absolute thresholds, another edge, the durations
    r = cwt.detect(dm.BAND, units="absolute", threshold=3.0, edge=1.5)
    assert _exactly_the_model(cwt, r, "envelope", 1, ts, 3.0, 1.5, "absolute") == 8
    r = cwt.detect(dm.BAND, threshold=2.5, edge=1.0, min_duration=0.03, max_duration=0.2)
    assert _exactly_the_model(cwt, r, "envelope", 1, ts, 2.5, 1.0, "sd", min_duration=0.03, max_duration=0.2) == 8
    assert len(cwt.detect(dm.BAND, min_duration=1.0)) == 0 and len(cwt.detect(dm.BAND, max_duration=0.001)) == 0
    none = cwt.detect(dm.BAND, units="absolute", threshold=1e6, edge=1e6)                 # no run at all
    assert len(none) == 0 and none.n_candidates.tolist() == [0, 0] and none.start.dtype == np.float64
    # what triggered() takes (20 ms either side: the burst that ends 30 ms before the first epoch does keeps its window inside it)
    trig = cwt.triggered(r.peak_time[r.channel == 0], before=0.02, after=0.02)
    assert trig.n_events == 4 and trig.events_used.all()


def test_detect_after_the_single_channel_call(recorded):
    from ghost_amd.wave import ContinuousWaveletTransform
    x, ts = recorded["x"], recorded["ts"]
    one = ContinuousWaveletTransform()
    one.transform(x[1], fs=dm.FS, timestamps=ts, output="complex", dtype=np.float32, **dm.TRANSFORM)
    r, two = one.detect(dm.BAND), recorded[1].detect(dm.BAND)
    for name in ("mean", "sd", "lo", "hi", "n_columns", "n_candidates"):
        assert np.ndim(getattr(r, name)) == 0 and getattr(r, name) == getattr(two, name)[1], name
    assert r.channel.tolist() == [0] * 4
    for name in ("start", "stop", "peak_time", "peak", "start_col", "stop_col", "peak_col"):
        assert np.array_equal(getattr(r, name), getattr(two, name)[two.channel == 1]), name
    assert dm.found(r.channel, r.peak_time, r.start_col, r.stop_col, ts, 1, {0: dm.BURSTS[1]}) == []


def test_zero_columns_of_an_epoch_gap_are_not_counted_and_split_runs():
    """A plan with a gap between its epochs leaves exact zeros there: the statistics are those of the other columns, and with
    lo = 0 every epoch is one run that ends where the zeros begin."""
    from ghost_amd import engine
    from ghost_amd.wave import Morse
    x, _ = dm.recording()
    n, epochs = dm.N, [[0, 4000], [4200, dm.N]]
    f = 250.0 / 2 ** (np.arange(6) / 4)
    plan = engine.CwtPlan(n, 2, dm.FS, f, output="complex", epoch_bounds=epochs)
    result = plan.execute_resident(x)
    g, h = engine.band_weights(f, Morse(fs=dm.FS))
    res = engine.bandpass(result, engine.band_rows(dm.BAND, f), g, h, ("envelope",))
    trace = res.to_host()["envelope"][:, 0]
    assert not np.any(trace[:, 4000:4200]) and np.all(trace[:, :4000] > 0) and np.all(trace[:, 4200:] > 0)
    ptr = res.buffer.ptr.value + res._offsets()["envelope"]
    got = engine.trace_stats(ptr, res.pitch, 2, n)
    assert got[0].tolist() == [n - 200] * 2
    _check_stats(got, trace, "two epochs")
    live = np.concatenate([trace[:, :4000], trace[:, 4200:]], axis=1)
    assert np.all(np.abs(got[1] - live.astype(np.float64).mean(axis=1)) <= 1e-12)
    zero = engine.trace_runs(ptr, res.pitch, 2, n, np.zeros(2, np.float32))
    assert zero["start"].tolist() == [0, 4200] * 2 and zero["stop"].tolist() == [4000, n] * 2
    lo = got[1].astype(np.float32)
    runs = engine.trace_runs(ptr, res.pitch, 2, n, lo)
    _same_runs(runs, dm.model_runs(trace, lo), "two epochs")
    assert not np.any((runs["stop"] > 4000) & (runs["start"] < 4200))
    res.free()
    result.free()
    plan.close()


# -- 4. side effects -------------------------------------------------------------------------------------------------------
def test_the_resident_result_and_the_device_memory_are_as_they_were(recorded, monkeypatch):
    from ghost_amd import _lib, engine
    cwt = recorded[1]
    before = cwt.fetch()
    lazy = cwt._pending
    first = cwt.detect(dm.BAND)                                             # (whatever the first call sets up once is set up)
    # every device buffer the Python layer makes from here on is freed by the time the call returns or raises ...
    made = []

    class Tracked(engine.DeviceBuffer):
        def __init__(self, nbytes):
            super().__init__(nbytes)
            made.append(self)

    monkeypatch.setattr(engine, "DeviceBuffer", Tracked)
    free = engine.device_memory()[0]
    leak = 2 * engine._pitch(dm.N) * 4                                      # ... and so says the device: the trace alone, kept 32 times, is 2 MiB
    assert 32 * leak >= 2 << 20

    def settled(n_buffers):
        assert len(made) == n_buffers and not any(b.ptr for b in made), [b.nbytes for b in made if b.ptr]
        assert abs(engine.device_memory()[0] - free) < 1 << 20
        del made[:]

    again = cwt.detect(dm.BAND, on="power")
    settled(2)                                                              # the trace and the runs
    again = cwt.detect(dm.BAND)
    settled(2)
    for name in ("channel", "start", "stop", "peak_time", "peak", "start_col", "stop_col", "peak_col", "mean", "sd", "lo", "hi"):
        assert getattr(first, name).tobytes() == getattr(again, name).tobytes(), name
    # the temporaries are freed when a step raises: a threshold that is not finite reaches gcwt_trace_runs
    real = engine.trace_runs
    monkeypatch.setattr(engine, "trace_runs", lambda ptr, pitch, c, n, lo: real(ptr, pitch, c, n, np.full(c, np.nan, np.float32)))
    for _ in range(32):
        with pytest.raises(_lib.GhostCwtError, match=r"gcwt_trace_runs: lo\[0\]"):
            cwt.detect(dm.BAND)
    settled(32)
    monkeypatch.setattr(engine, "trace_runs", real)
    with pytest.raises(ValueError, match="hi < lo"):                        # a refusal: before any device work
        cwt.detect(dm.BAND, threshold=1.0, edge=2.0)
    settled(0)
    for _ in range(32):
        with pytest.raises(ValueError, match="lo >= 0"):                    # ... and one that needs the statistics: after them, all is freed
            cwt.detect(dm.BAND, threshold=-1.0, edge=-1.5)
    settled(32)
    assert cwt._pending is lazy
    assert cwt.fetch().tobytes() == before.tobytes()
    assert len(cwt.detect(dm.BAND)) == len(first)


def test_error_surface_on_the_device():
    from ghost_amd.synthetic import lfp
    from ghost_amd.wave import ContinuousWaveletTransform
    x = lfp(4, 4096, dm.FS, seed=1)
    kw = dict(fs=dm.FS, freq_limits=[20, 200], voices_per_octave=4)
    cwt = ContinuousWaveletTransform()
    cwt.transform(x, multichannel=True, **kw)                                            # amplitude
    with pytest.raises(ValueError, match="complex"):
        cwt.detect((20.0, 60.0))
    cwt = ContinuousWaveletTransform()
    cwt.transform(x, multichannel=True, output="complex", devices=[0, 0], **kw)          # sharded
    with pytest.raises(ValueError, match="devices"):
        cwt.detect((20.0, 60.0))
    cwt = ContinuousWaveletTransform()
    cwt.transform(x, multichannel=True, output="complex", **kw)
    with pytest.raises(ValueError, match=r"bands\[0\]"):
        cwt.detect((1.0, 4.0))                                                            # a band with no rows
    with pytest.raises(ValueError, match="'on'"):
        cwt.detect((20.0, 60.0), on="analytic")
    r = cwt.detect((20.0, 60.0))                                                          # ... and it still works
    assert r.mean.shape == (4,) and r.n_columns.tolist() == [4096] * 4
    cwt.release_device()
    with pytest.raises(ValueError, match="transform"):
        cwt.detect((20.0, 60.0))
