"""gcwt_trace_order on the MI355X (csrc/trace_order.hip; include/ghostcwt.h has the definition) and what is built on it:
the order statistics of uploaded traces byte for byte against the NumPy model (tests/order_model.py) at every size where a
tile, a chunk or a pass of the select could go wrong, with and without centres, at every alignment; engine.trace_median_mad
against the model and NumPy's median; detect(stats='median') and detect(baseline=...) end to end against the definition
applied to bandpass()'s own trace; the device's memory.  No tolerance anywhere but for mean and sd, whose bound
detect_model derives."""
import numpy as np
import pytest

import detect_model as dm
import order_model as om

pytestmark = pytest.mark.gpu

T = 1024                                            # GCWT_RUNS_TILE_COLS
Q = 8192                                            # GCWT_ORDER_CHUNK_COLS
SIZES = (1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T, 3 * T + 1, Q - 1, Q, Q + 1, 2 * Q + 3)


def _f(bits):
    return np.array(bits, np.uint32).view(np.float32)


def _pitch(n):
    from ghost_amd.engine import _pitch
    return _pitch(n)


def _upload(traces, pitch):
    """(C, n) float32 traces on the device, pitch elements apart; what lies between n and pitch is +inf: read perhaps,
    never counted."""
    from ghost_amd.engine import DeviceBuffer
    traces = np.asarray(traces, dtype=np.float32)
    c, n = traces.shape
    padded = np.full((c, pitch), np.inf, np.float32)
    padded[:, :n] = traces
    buf = DeviceBuffer(padded.nbytes)
    buf.upload(padded)
    return buf


def _cases(n, rng):
    """(traces (C, n), centres (C,)): traces that differ in n, each one a way for a pass of the select to go wrong."""
    rows, centres = [], []

    def add(v, centre):
        rows.append(np.asarray(v, dtype=np.float32)), centres.append(np.float32(centre))

    noise = rng.standard_normal(n).astype(np.float32)
    add(noise, noise[n // 2])                                               # a centre equal to a value: key +0, included
    add(np.full(n, 1.5), 1.5)                                               # all equal: one bin in every pass; every key +0
    add(_f([0x3f800000, 0x3f800001])[rng.integers(0, 2, n)], 1e4)           # the lowest mantissa bit: the last pass decides; a far centre rounds
    add(_f([0x3f800000, 0x3f801000])[rng.integers(0, 2, n)], 1.0)           # a bit of the middle digit alone
    add(np.array([-1.0, 2.0, 5.0])[rng.integers(0, 3, n)], 2.0)             # three values, many ties
    holes = rng.standard_normal(n)
    holes[rng.random(n) < 0.3] = 0.0                                        # zeros of both signs are excluded
    holes[rng.random(n) < 0.1] = -0.0
    add(holes, 1e8)
    add(np.zeros(n), 0.5)                                                   # n = 0 between two others
    special = rng.standard_normal(n).astype(np.float32)
    for value in (_f(0x7fc00000), _f(0xffc00000), _f(0x7fc01234), _f(0xffc00001), np.inf, -np.inf):
        special[rng.random(n) < 0.04] = value
    add(special, 0.25)
    add(np.array([1e-40, -1e-40, 3e-41, 3e-40, 1.0, 0.0])[rng.integers(0, 6, n)], 2e-40)   # subnormals, and subnormal differences
    add(rng.standard_normal(n) * 1e-3 + 7.0, -3.0)                          # a narrow trace: everything in two top bins
    return np.stack(rows), np.array(centres, np.float32)


def _ranks(traces, n_cols):
    """Per trace 0, n - 1, (n - 1) // 2 and n // 2 of its own n; in the trace with holes a rank >= n beside valid ones."""
    cnt = np.array([np.count_nonzero(v != 0) for v in traces], np.int64)
    ranks = np.stack((np.zeros_like(cnt), np.maximum(cnt - 1, 0), np.maximum(cnt - 1, 0) // 2, cnt // 2), axis=1)
    ranks[5, 1] = n_cols
    return ranks


def _same(got, want, msg):
    assert got[0].dtype == np.int64 and got[1].dtype == np.float32 and got[1].shape == want[1].shape, msg
    assert np.array_equal(got[0], want[0]), (msg, got[0], want[0])
    assert got[1].tobytes() == want[1].tobytes(), (msg, got[1].view(np.uint32), want[1].view(np.uint32))


@pytest.mark.parametrize("n", SIZES)
def test_order_statistics_are_the_models_byte_for_byte(n):
    from ghost_amd import engine
    traces, centres = _cases(n, np.random.default_rng(n))
    c, pitch, ranks = traces.shape[0], _pitch(n), _ranks(traces, n)
    buf = _upload(traces, pitch)
    try:
        for centre in (None, centres):
            want = om.model_order(traces, ranks, centre)
            assert want[0][6] == 0 and want[1][6].view(np.uint32).tolist() == [0x7fc00000] * 4
            assert want[1][5, 1].view(np.uint32) == 0x7fc00000
            _same(engine.trace_order(buf.ptr, pitch, c, n, ranks, centre), want, ("four ranks", centre is not None))
            for j in range(4):
                _same(engine.trace_order(buf.ptr, pitch, c, n, ranks[:, j:j + 1], centre), (want[0], want[1][:, j:j + 1]),
                      ("one rank", j, centre is not None))
        # ranks (R,) go to every trace
        shared = np.array([0, n // 2, n])
        _same(engine.trace_order(buf.ptr, pitch, c, n, shared), om.model_order(traces, shared), "broadcast")
        # median and MAD
        got, want = engine.trace_median_mad(buf.ptr, pitch, c, n), om.model_median_mad(traces)
        for g, w, name in zip(got, want, ("n", "median", "mad")):
            assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (name, g, w)
    finally:
        buf.free()


@pytest.mark.parametrize("n", (5, 65, T + 1, Q + 1))
def test_padding_pitch_and_alignment(n):
    """+inf in the padding is never counted; an odd pitch and a trace pointer 1, 2 and 3 columns into the buffer -- the path
    baseline= takes -- read every column one by one."""
    from ghost_amd import engine
    traces, centres = _cases(n, np.random.default_rng(100 + n))
    c = traces.shape[0]
    for pitch in (_pitch(n), n, (n + 2) | 1, n + 6):
        buf = _upload(traces, pitch)
        try:
            for k in (0, 1, 2, 3):
                if n - k < 1:
                    continue
                part = traces[:, k:]
                ranks = _ranks(part, n - k)
                for centre in (None, centres):
                    got = engine.trace_order(buf.ptr.value + 4 * k, pitch, c, n - k, ranks, centre)
                    _same(got, om.model_order(part, ranks, centre), (pitch, k, centre is not None))
                    assert not np.any(np.isposinf(got[1][[0, 1, 2, 3, 4, 5, 8, 9]]))       # (traces without an inf of their own)
        finally:
            buf.free()


def test_a_trace_gives_the_same_bytes_alone_among_others_and_again():
    from ghost_amd import engine
    n = 2 * Q + 3
    traces, centres = _cases(n, np.random.default_rng(5))
    c, pitch, ranks = traces.shape[0], _pitch(n), _ranks(traces, n)
    buf = _upload(traces, pitch)
    try:
        for centre in (None, centres):
            first = engine.trace_order(buf.ptr, pitch, c, n, ranks, centre)
            _same(engine.trace_order(buf.ptr, pitch, c, n, ranks, centre), first, "second call")
            for i in range(c):
                alone = engine.trace_order(buf.ptr.value + i * pitch * 4, pitch, 1, n, ranks[i:i + 1], None if centre is None else centre[i:i + 1])
                _same(alone, (first[0][i:i + 1], first[1][i:i + 1]), ("alone", i))
            # fewer columns of the same buffer: what lies past n_cols is not counted
            m = Q + 5
            part = traces[:, :m]
            _same(engine.trace_order(buf.ptr, pitch, c, m, _ranks(part, m), centre), om.model_order(part, _ranks(part, m), centre), "first columns")
    finally:
        buf.free()


def test_median_and_mad_of_a_long_trace_are_numpys():
    from ghost_amd import engine
    n = 70 * 1024 + 3
    rng = np.random.default_rng(9)
    traces = np.stack([rng.standard_normal(n) + 3.0, np.abs(rng.standard_normal(n)) ** 2, rng.standard_normal(n - 1).tolist() + [0.0]]).astype(np.float32)
    buf = _upload(traces, _pitch(n))
    try:
        cnt, median, mad = engine.trace_median_mad(buf.ptr, _pitch(n), 3, n)
    finally:
        buf.free()
    want = om.model_median_mad(traces)
    assert cnt.tolist() == [n, n, n - 1] == want[0].tolist()
    assert median.tobytes() == want[1].tobytes() and mad.tobytes() == want[2].tobytes()
    for i in range(3):
        v = traces[i][traces[i] != 0]
        assert median[i] == np.median(v.astype(np.float64))
        assert mad[i] == np.median(np.abs(v - np.float32(median[i])).astype(np.float64))


# -- detect(stats='median'), detect(baseline=...) ----------------------------------------------------------------------------
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


def _exactly_the_model(cwt, r, on, stride, ts, stats, threshold, edge, cols=None):
    """detect()'s report and events against the definitions applied on the host to bandpass()'s own trace; the statistics
    over the columns ``cols`` = (c0, c1), the runs over all."""
    trace = getattr(cwt.bandpass(dm.BAND, outputs=(on,)), on)[:, 0]
    t = ts[::stride]
    part = trace if cols is None else trace[:, cols[0]:cols[1]]
    for ch in range(trace.shape[0]):
        cnt, m, s = dm.model_stats(part[ch])
        bm, bs = dm.stats_bound(part[ch])
        assert r.n_columns[ch] == cnt == part.shape[1]
        assert abs(r.mean[ch] - m) <= bm and abs(r.sd[ch] - s) <= bs, (ch, r.mean[ch] - m, bm, r.sd[ch] - s, bs)
    if stats == "median":
        cnt, median, mad = om.model_median_mad(part)
        assert r.median.dtype == r.mad.dtype == np.float64
        assert r.median.tobytes() == median.tobytes() and r.mad.tobytes() == mad.tobytes(), (r.median, median, r.mad, mad)
        centre, spread = median, 1.482602218505602 * mad
    else:
        assert r.median is None and r.mad is None
        centre, spread = r.mean, r.sd
    hi, lo = (centre + threshold * spread).astype(np.float32), (centre + edge * spread).astype(np.float32)
    assert r.lo.dtype == r.hi.dtype == np.float32 and r.hi.tobytes() == hi.tobytes() and r.lo.tobytes() == lo.tobytes()
    runs = dm.model_runs(trace, lo)
    assert np.array_equal(r.n_candidates, runs["counts"])
    want = dm.model_events(runs, hi, t, 0.0, 0.0, None, stride / dm.FS)
    for name, mine in (("trace", r.channel), ("start", r.start_col), ("stop", r.stop_col), ("peak_col", r.peak_col), ("peak", r.peak)):
        assert mine.dtype == want[name].dtype and mine.tobytes() == want[name].tobytes(), name
    assert np.array_equal(r.start, t[r.start_col]) and np.array_equal(r.stop, t[r.stop_col - 1]) and np.array_equal(r.peak_time, t[r.peak_col])
    assert r.baseline_cols == cols
    return trace


@pytest.mark.parametrize("on,stride", [("envelope", 1), ("power", 1), ("envelope", 4), ("power", 4)])
def test_detect_on_median_and_mad_is_the_definition_and_finds_the_bursts(recorded, on, stride):
    cwt, ts = recorded[stride], recorded["ts"]
    r = cwt.detect(dm.BAND, on=on, stats="median", threshold=12, edge=2)
    _exactly_the_model(cwt, r, on, stride, ts, "median", 12.0, 2.0)
    print("%s, stride %d: %d events of %s candidates; median %s mad %s; mean %s sd %s" % (on, stride, len(r), r.n_candidates, r.median, r.mad, r.mean, r.sd))
    assert dm.found(r.channel, r.peak_time, r.start_col, r.stop_col, ts, stride) == []
    assert r.channel.tolist() == [0] * 4 + [1] * 4
    # the defaults are today's call; stats with absolute units changes no threshold
    plain, same = cwt.detect(dm.BAND, on=on), cwt.detect(dm.BAND, on=on, stats="mean", baseline=None)
    assert plain.median is None and plain.baseline_cols is None
    for name in ("channel", "start", "stop", "peak_time", "peak", "start_col", "stop_col", "peak_col", "mean", "sd", "lo", "hi", "n_columns", "n_candidates"):
        assert getattr(plain, name).tobytes() == getattr(same, name).tobytes(), name
    a, b = cwt.detect(dm.BAND, on=on, units="absolute", threshold=3.0, edge=1.5), cwt.detect(dm.BAND, on=on, units="absolute", threshold=3.0, edge=1.5, stats="median")
    for name in ("channel", "start_col", "stop_col", "peak_col", "peak", "lo", "hi"):
        assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), name
    assert b.median.tobytes() == r.median.tobytes() and b.mad.tobytes() == r.mad.tobytes()


@pytest.mark.parametrize("stride", (1, 4))
def test_detect_with_a_baseline_interval(recorded, stride):
    cwt, ts = recorded[stride], recorded["ts"]
    n = -(-dm.N // stride)
    split = dm.SPLIT // stride
    second = (ts[dm.SPLIT], ts[-1] + 1.0)                                   # the second epoch
    inside = (ts[dm.SPLIT] + 0.0005, ts[dm.SPLIT] + 3.0)                    # ... and a stretch of it that starts off 16 bytes
    c0 = split + 1
    c1 = split + int(np.count_nonzero(ts[dm.SPLIT::stride] < inside[1]))
    assert (c0 * 4) % 16 != 0
    for interval, cols in ((second, (split, n)), (inside, (c0, c1))):
        for stats in ("median", "mean"):
            for on in ("envelope", "power"):
                threshold, edge = (12.0, 2.0) if stats == "median" else (3.0, 0.0)
                r = cwt.detect(dm.BAND, on=on, stats=stats, threshold=threshold, edge=edge, baseline=interval)
                _exactly_the_model(cwt, r, on, stride, ts, stats, threshold, edge, cols)
    # the whole clock is no baseline at all
    whole = cwt.detect(dm.BAND, stats="median", threshold=12, edge=2, baseline=(ts[0], ts[-1] + 1.0))
    none = cwt.detect(dm.BAND, stats="median", threshold=12, edge=2)
    assert whole.baseline_cols == (0, n) and none.baseline_cols is None
    for name in ("channel", "start_col", "stop_col", "peak_col", "peak", "lo", "hi", "median", "mad", "mean", "sd"):
        assert getattr(whole, name).tobytes() == getattr(none, name).tobytes(), name
    with pytest.raises(ValueError, match=r"^detect\(\): 'baseline'"):
        cwt.detect(dm.BAND, baseline=(ts[dm.SPLIT - 1] + 0.5, ts[dm.SPLIT] - 0.5))       # inside the gap between the epochs: no column


def test_detect_after_the_single_channel_call(recorded):
    from ghost_amd.wave import ContinuousWaveletTransform
    x, ts = recorded["x"], recorded["ts"]
    one = ContinuousWaveletTransform()
    one.transform(x[1], fs=dm.FS, timestamps=ts, output="complex", dtype=np.float32, **dm.TRANSFORM)
    kw = dict(stats="median", threshold=12, edge=2, baseline=(ts[dm.SPLIT], ts[-1] + 1.0))
    r, two = one.detect(dm.BAND, **kw), recorded[1].detect(dm.BAND, **kw)
    one.release_device()
    for name in ("median", "mad", "mean", "sd", "lo", "hi", "n_columns", "n_candidates"):
        assert np.ndim(getattr(r, name)) == 0 and getattr(r, name) == getattr(two, name)[1], name
    assert r.baseline_cols == two.baseline_cols == (dm.SPLIT, dm.N)
    assert r.channel.tolist() == [0] * 4
    for name in ("start", "stop", "peak_time", "peak", "start_col", "stop_col", "peak_col"):
        assert np.array_equal(getattr(r, name), getattr(two, name)[two.channel == 1]), name


def test_the_device_memory_is_as_it_was(recorded, monkeypatch):
    from ghost_amd import engine
    cwt = recorded[1]
    kw = dict(stats="median", threshold=12, edge=2)
    first = cwt.detect(dm.BAND, **kw)                                       # (whatever the first call sets up once is set up)
    made = []

    class Tracked(engine.DeviceBuffer):
        def __init__(self, nbytes):
            super().__init__(nbytes)
            made.append(self)

    monkeypatch.setattr(engine, "DeviceBuffer", Tracked)
    free = engine.device_memory()[0]
    leak = 2 * engine._pitch(dm.N) * 4                                      # the trace alone, kept 32 times, is 2 MiB
    assert 32 * leak >= 2 << 20

    def settled(n_buffers):
        assert len(made) == n_buffers and not any(b.ptr for b in made), [b.nbytes for b in made if b.ptr]
        assert abs(engine.device_memory()[0] - free) < 1 << 20
        del made[:]

    again = cwt.detect(dm.BAND, **kw)
    settled(2)                                                              # the trace and the runs
    for name in ("channel", "start_col", "stop_col", "peak_col", "peak", "median", "mad", "lo", "hi"):
        assert getattr(first, name).tobytes() == getattr(again, name).tobytes(), name
    # a step in the middle raises -- the third select, whose centre is not finite: the trace is freed
    real = engine.trace_order

    def broken(ptr, pitch, c, n, ranks, center=None):
        return real(ptr, pitch, c, n, ranks, None if center is None else np.full(c, np.nan, np.float32))

    monkeypatch.setattr(engine, "trace_order", broken)
    for _ in range(32):
        with pytest.raises(ValueError, match="'center' must be finite"):
            cwt.detect(dm.BAND, **kw)
    settled(32)
    monkeypatch.setattr(engine, "trace_order", real)
    for _ in range(32):
        with pytest.raises(ValueError, match="lo >= 0"):                    # one that needs the statistics: after them, all is freed
            cwt.detect(dm.BAND, stats="median", threshold=-1.0, edge=-30.0)
    settled(32)
    with pytest.raises(ValueError, match="'stats'"):                        # a refusal: before any device work
        cwt.detect(dm.BAND, stats="robust")
    settled(0)
    assert len(cwt.detect(dm.BAND, **kw)) == len(first)
