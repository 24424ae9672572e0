"""gcwt_trace_smooth and detect(smooth=, combine=) on the MI355X (csrc/trace_smooth.hip, include/ghostcwt.h): the impulse
response bit for bit, uploaded traces against the float64 model within the bound it derives (tests/smooth_model.py) at
every size, kernel length and pitch where the tiling, the halo or the loads could go wrong, segments bit for bit against
the same columns smoothed alone, the member mean bit for bit, detect() end to end -- exactly the definition applied to the
device's own smoothed trace, and physically on a recording whose bursts the model is known to find
(tests/test_smooth_host.py) -- and its side effects."""
import numpy as np
import pytest

import detect_model as dm
import smooth_model as sm

pytestmark = pytest.mark.gpu

T = 1024                                            # GCWT_SMOOTH_TILE_COLS
LIMIT = 4096                                        # GCWT_SMOOTH_MAX_HALF
SIZES = (1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T, 3 * T + 1)
HALVES = (0, 1, 2, 3, 5, 16, 63, 64, 65, 255, T, T + 1)


def _pitch(n):
    from ghost_amd.engine import _pitch
    return _pitch(n)


def _upload(traces, pitch):
    """(C, n) float32 traces on the device, pitch elements apart; what lies between n and pitch is +inf: read perhaps,
    never used."""
    from ghost_amd.engine import DeviceBuffer
    traces = np.asarray(traces, dtype=np.float32)
    c, n = traces.shape
    padded = np.full((c, pitch), np.inf, np.float32)
    padded[:, :n] = traces
    buf = DeviceBuffer(padded.nbytes)
    buf.upload(padded)
    return buf


def _smooth(buf, pitch, c, n, taps, segments=None, members=None, first=0):
    """engine.trace_smooth on the columns first .. first + n of an uploaded buffer -> (rows, n) float32 on the host."""
    from ghost_amd import engine
    out, out_pitch, shape = engine.trace_smooth(buf.ptr.value + 4 * first, pitch, c, n, taps, segments, members)
    try:
        assert shape == ((1 if members is not None else c), n) and out_pitch >= n and out.nbytes == shape[0] * out_pitch * 4
        return out.download((shape[0], out_pitch), np.float32)[:, :n].copy()
    finally:
        out.free()


def _odd(n):
    return n + 1 if n % 2 == 0 else n + 2


def _within(got, traces, taps, segments, msg):
    """Every trace of ``got`` against the model: finite columns within the derived bound, a NaN exactly where the model has
    one.  -> the worst error / bound."""
    worst = 0.0
    for i, v in enumerate(traces):
        want, room = sm.smooth(v, taps, segments), sm.bound(v, taps, segments)
        assert np.array_equal(np.isnan(got[i]), np.isnan(want)), (msg, i, np.flatnonzero(np.isnan(got[i]) != np.isnan(want))[:8])
        bad = ~np.isfinite(want)                                            # an inf in the window: the same inf, or the same NaN
        assert np.array_equal(got[i][np.isinf(want)], want[np.isinf(want)]), (msg, i)
        err = np.abs(got[i].astype(np.float64)[~bad] - want[~bad])
        assert np.all(err <= room[~bad]), (msg, i, int(np.argmax(err - room[~bad])), err.max(), room[~bad].max())
        if err.size and room[~bad].max() > 0:
            worst = max(worst, float(np.max(err[room[~bad] > 0] / room[~bad][room[~bad] > 0])))
    return worst


# -- 1. the impulse response -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", (1, 5, 64, 300, T + 1))
def test_impulse_response_is_the_taps_bit_for_bit(half):
    n, edge = 3 * T + 1, T + 37
    segments = np.array([[0, edge], [edge, n]])
    at = (0, 1, T - 1, T, edge - 1, edge, n - 1)
    traces = np.zeros((len(at), n), np.float32)
    traces[np.arange(len(at)), at] = 1
    w = sm.taps_of_half(half)
    kernel = np.concatenate((w[:0:-1], w))
    buf = _upload(traces, _pitch(n))
    for segs in (None, segments):
        got = _smooth(buf, _pitch(n), len(at), n, w, segs)
        for i, c in enumerate(at):
            a, b = (0, n) if segs is None else next((a, b) for a, b in segs if a <= c < b)
            want = np.zeros(n, np.float32)
            lo, hi = max(a, c - half), min(b, c + half + 1)
            want[lo:hi] = kernel[lo - (c - half):hi - (c - half)]
            assert got[i].tobytes() == want.tobytes(), (half, segs is None, c, np.flatnonzero(got[i] != want)[:8])
    buf.free()


# -- 2. against the model, within the bound -------------------------------------------------------------------------------
def _traces(n, rng):
    """random, all ones, and a random trace with one NaN (at the middle and, where there is room, beside column 0)."""
    rows = [rng.standard_normal(n) * 3 + 1, np.ones(n), rng.standard_normal(n)]
    rows[2][n // 2] = np.nan
    if n > 70:
        rows.append(rng.standard_normal(n))
        rows[3][1] = np.nan
        rows[3][n - 1] = np.nan
    return np.stack(rows).astype(np.float32)


@pytest.mark.parametrize("n", SIZES)
def test_traces_meet_the_model_within_the_derived_bound(n):
    traces = _traces(n, np.random.default_rng(n))
    c = len(traces)
    worst = 0.0
    for pitch in (_pitch(n), _odd(n), n):
        buf = _upload(traces, pitch)
        for half in HALVES + ((LIMIT,) if n == 2 * T and pitch == _pitch(n) else ()):
            w = sm.taps_of_half(half)
            got = _smooth(buf, pitch, c, n, w)
            worst = max(worst, _within(got, traces, w, None, "n=%d pitch=%d half=%d" % (n, pitch, half)))
            # the NaN reaches exactly the columns within half of it
            assert np.array_equal(np.isnan(got[2]), sm.reach(np.isnan(traces[2]), half, n)), (n, pitch, half)
            if half == 0:
                assert got.tobytes() == traces.tobytes()                     # w_0 = 1: the identity
        buf.free()
    print("n=%d: worst error / bound %.3g" % (n, worst))


# -- 3. segments -----------------------------------------------------------------------------------------------------------
N3 = 3 * T + 1
COVER = np.array([[0, 1], [1, T - 1], [T - 1, T], [T, T + 1], [T + 1, N3 - 1], [N3 - 1, N3]])         # edges at 1, T - 1, T, T + 1, n - 1
HOLES = np.array([[3, 10], [12, 13], [40, T + 20], [T + 50, 2 * T - 5], [2 * T + 300, N3 - 7]])        # uncovered before, between, after


@pytest.mark.parametrize("half", (0, 3, 64, 300, T + 1))
def test_segments_never_see_their_neighbours(half):
    rng = np.random.default_rng(half)
    traces = (rng.standard_normal((3, N3)) + 2).astype(np.float32)
    traces[1, T + 20] = np.nan                                              # the first column past a segment of HOLES ...
    traces[1, T + 49] = np.inf                                              # ... and the last before the next: never seen
    traces[2, T] = np.nan                                                   # a one-column segment of COVER, all of it NaN
    pitch = _pitch(N3)
    buf = _upload(traces, pitch)
    w = sm.taps_of_half(half)
    for name, segs in (("cover", COVER), ("holes", HOLES)):
        got = _smooth(buf, pitch, 3, N3, w, segs)
        _within(got, traces, w, segs, "%s half=%d" % (name, half))
        covered = np.zeros(N3, bool)
        for a, b in segs:
            covered[a:b] = True
        assert not got[:, ~covered].view(np.uint32).any(), name           # exact +0, whatever the trace holds there
        if name == "holes":
            assert np.isfinite(got[1]).all()                                # the NaN and the inf lie in no segment
        else:
            assert np.array_equal(np.isnan(got[2]), np.arange(N3) == T)
        # each segment is the same columns smoothed alone: a trace of their own, through a pointer offset (which is off 16
        # bytes for most of them)
        for a, b in segs.tolist():
            alone = _smooth(buf, pitch, 3, b - a, w, None, None, first=a)
            assert alone.tobytes() == np.ascontiguousarray(got[:, a:b]).tobytes(), (name, half, a, b)
    # an edge inside a tile's halo only: the tile [T, 2T) with a segment ending at 2T + 3
    segs = np.array([[T - 2, 2 * T + 3], [2 * T + 3, N3]])
    got = _smooth(buf, pitch, 3, N3, w, segs)
    _within(got, traces, w, segs, "halo half=%d" % half)
    buf.free()


# -- 4. company --------------------------------------------------------------------------------------------------------------
def test_bits_do_not_depend_on_company():
    n = 2 * T + 37
    traces = (np.random.default_rng(4).standard_normal((5, n)) * 2).astype(np.float32)
    pitch = _pitch(n)
    buf = _upload(traces, pitch)
    segs = np.array([[0, 700], [700, n - 3]])
    for half in (2, 65, T + 1):
        w = sm.taps_of_half(half)
        first = _smooth(buf, pitch, 5, n, w, segs)
        assert _smooth(buf, pitch, 5, n, w, segs).tobytes() == first.tobytes(), "second call"
        for i in range(5):
            alone = _smooth(buf, pitch, 1, n, w, segs, None, first=i * pitch)
            assert alone.tobytes() == first[i:i + 1].tobytes(), ("alone", half, i)
        # the same buffer seen with fewer columns: the first segment is as it was
        short = _smooth(buf, pitch, 5, 900, w, np.array([[0, 700], [700, 900]]))
        assert np.ascontiguousarray(short[:, :700]).tobytes() == np.ascontiguousarray(first[:, :700]).tobytes()
    buf.free()
    from ghost_amd import engine
    with pytest.raises(ValueError, match="freed"):
        engine.trace_smooth(buf.ptr, pitch, 5, n, w)


# -- 5. combine ----------------------------------------------------------------------------------------------------------------
MEMBERS = ([3], [0, 1], [2, 0, 5], [0, 1, 2, 3, 4, 5, 6], [1, 1], [4, 0, 4, 4], [6, 5, 4, 3, 2, 1, 0], [5, 2, 0])


def test_combine_is_the_models_chain_bit_for_bit():
    rng = np.random.default_rng(5)
    for n in (65, T + 1, 2 * T + 5):
        traces = (rng.standard_normal((7, n)) * np.array([1, 1e3, 1e-3, 7, 1, 30, 1])[:, None]).astype(np.float32)
        traces[6, n // 3] = np.inf
        for pitch in (_pitch(n), _odd(n), n):
            buf = _upload(traces, pitch)
            for members in MEMBERS:
                want = sm.combine(traces, members)
                got = _smooth(buf, pitch, 7, n, np.ones(1, np.float32), None, members)
                assert got.shape == (1, n) and got[0].tobytes() == want.tobytes(), (n, pitch, members)
                # then smoothed: the model's smoother on the model's mean, within the bound (members of finite traces)
                if 6 not in members:
                    for half in (3, 64, T + 1):
                        w = sm.taps_of_half(half)
                        segs = np.array([[0, n // 2], [n // 2, n]])
                        _within(_smooth(buf, pitch, 7, n, w, segs, members), want[None], w, segs, (n, pitch, members, half))
            buf.free()


# -- 6. end to end -----------------------------------------------------------------------------------------------------------
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


SMOOTH = 0.004
EVERYTHING = {-1: tuple(sorted(dm.BURSTS[0] + dm.BURSTS[1]))}


def _device_trace(cwt, on, stride, ts, smooth, combine):
    """What detect(smooth=, combine=) thresholds: bandpass, then trace_smooth, brought to the host."""
    from ghost_amd import engine
    from ghost_amd.wave import Morse
    f = np.array(cwt.frequencies)
    g, h = engine.band_weights(f, Morse(fs=dm.FS))
    res = engine.bandpass(cwt._device_result, engine.band_rows(dm.BAND, f), g, h, (on,))
    t = ts[::stride]
    try:
        c, n = res.n_channels, res.n_cols
        taps = np.ones(1, np.float32) if smooth is None else engine.smooth_taps(smooth * dm.FS / stride)
        out, pitch, shape = engine.trace_smooth(res.buffer.ptr.value + res._offsets()[on], res.pitch, c, n, taps,
                                                engine.segments_of(t, stride / dm.FS, dm.FS, n), np.arange(c) if combine else None)
        try:
            return out.download((shape[0], pitch), np.float32)[:, :n].copy(), len(taps) - 1
        finally:
            out.free()
    finally:
        res.free()


def _axis(v, combine):
    return np.atleast_1d(v) if combine else v


def _exactly_the_model(r, trace, stride, ts, combine, threshold=3.0, edge=0.0):
    """detect()'s result against the definition applied on the host to the device's own smoothed trace."""
    from ghost_amd import engine
    t = ts[::stride]
    mean, sd, lo, hi = (_axis(getattr(r, k), combine) for k in ("mean", "sd", "lo", "hi"))
    for ch in range(trace.shape[0]):
        cnt, m, s = dm.model_stats(trace[ch])
        bm, bs = dm.stats_bound(trace[ch])
        assert _axis(r.n_columns, combine)[ch] == cnt == trace.shape[1]
        assert abs(mean[ch] - m) <= bm and abs(sd[ch] - s) <= bs, (ch, mean[ch] - m, bm, sd[ch] - s, bs)
    assert lo.dtype == hi.dtype == np.float32
    assert np.array_equal(hi, (mean + threshold * sd).astype(np.float32)) and np.array_equal(lo, (mean + edge * sd).astype(np.float32))
    runs = dm.model_runs(trace, lo)
    assert np.array_equal(_axis(r.n_candidates, combine), runs["counts"])
    want = engine.event_filter(runs["trace"], runs["start"], runs["stop"], runs["peak_col"], runs["peak"], hi, t, 0.0, 0.0, None,
                               stride / dm.FS)
    loop = dm.model_events(runs, hi, t, 0.0, 0.0, None, stride / dm.FS)
    assert want["trace"].tobytes() == loop["trace"].tobytes()
    channel = np.full_like(want["trace"], -1) if combine else want["trace"]
    assert r.channel.dtype == channel.dtype and r.channel.tobytes() == channel.tobytes()
    for name, mine in (("start", r.start_col), ("stop", r.stop_col), ("peak_col", r.peak_col), ("peak", r.peak)):
        assert mine.dtype == want[name].dtype and mine.tobytes() == want[name].tobytes() == loop[name].tobytes(), name
    assert np.array_equal(r.start, t[r.start_col]) and np.array_equal(r.stop, t[r.stop_col - 1]) and np.array_equal(r.peak_time, t[r.peak_col])
    assert np.array_equal(r.peak, trace[want["trace"], r.peak_col])
    if combine:
        assert all(np.ndim(getattr(r, k)) == 0 for k in ("mean", "sd", "lo", "hi", "n_columns", "n_candidates"))


@pytest.mark.parametrize("combine", (False, True))
@pytest.mark.parametrize("on,stride", [("envelope", 1), ("power", 1), ("envelope", 4), ("power", 4)])
def test_detect_is_the_definition_on_the_smoothed_trace_and_finds_the_bursts(recorded, on, stride, combine):
    """n_candidates: smoothing removes candidates -- except from the mean power trace, whose only runs above its mean are
    the 8 bursts before and after (tests/test_smooth_host.py settles both on the oracle's coefficients)."""
    cwt, ts = recorded[stride], recorded["ts"]
    r = cwt.detect(dm.BAND, on=on, smooth=SMOOTH, combine=combine)
    trace, half = _device_trace(cwt, on, stride, ts, SMOOTH, combine)
    assert (r.smooth, r.half, r.combined, half) == (SMOOTH, int(4 * SMOOTH * dm.FS / stride + 0.5), combine, r.half)
    assert trace.shape == ((1 if combine else 2), -(-dm.N // stride))
    _exactly_the_model(r, trace, stride, ts, combine)
    bursts = EVERYTHING if combine else dm.BURSTS
    assert dm.found(r.channel, r.peak_time, r.start_col, r.stop_col, ts, stride, bursts) == []
    assert len(r) == 8
    plain = cwt.detect(dm.BAND, on=on, combine=combine)
    assert (plain.smooth, plain.half, plain.combined) == (None, 0, combine)
    print("%s, stride %d, combine %s: %s candidates smoothed, %s not" % (on, stride, combine, r.n_candidates, plain.n_candidates))
    if (on, combine) == ("power", True):
        assert r.n_candidates == plain.n_candidates == 8
    else:
        assert np.sum(r.n_candidates) < np.sum(plain.n_candidates)
    if combine:                                                             # without smoothing: the mean trace itself
        raw, _ = _device_trace(cwt, on, stride, ts, None, True)
        _exactly_the_model(plain, raw, stride, ts, True)
        both = getattr(cwt.bandpass(dm.BAND, outputs=(on,)), on)[:, 0]
        assert raw[0].tobytes() == sm.combine(both, [0, 1]).tobytes()


def test_median_and_baseline_are_taken_on_the_smoothed_trace(recorded):
    from ghost_amd import engine
    cwt, ts = recorded[1], recorded["ts"]
    trace, _ = _device_trace(cwt, "envelope", 1, ts, SMOOTH, False)
    r = cwt.detect(dm.BAND, smooth=SMOOTH, stats="median")
    for ch in range(2):
        v = np.sort(trace[ch][trace[ch] != 0]).astype(np.float64)
        n = v.size
        median = (v[(n - 1) // 2] + v[n // 2]) / 2
        d = np.sort(np.abs(trace[ch][trace[ch] != 0] - np.float32(median))).astype(np.float64)
        assert r.median[ch] == median and r.mad[ch] == (d[(n - 1) // 2] + d[n // 2]) / 2, ch
    spread = engine.MAD_TO_SD * r.mad
    assert np.array_equal(r.hi, (r.median + 3.0 * spread).astype(np.float32)) and np.array_equal(r.lo, r.median.astype(np.float32))
    for r in (r, cwt.detect(dm.BAND, smooth=SMOOTH, stats="median", threshold=12.0, edge=2.0)):
        runs = dm.model_runs(trace, r.lo)
        assert np.array_equal(r.n_candidates, runs["counts"])
        want = dm.model_events(runs, r.hi, ts, 0.0, 0.0, None, 1 / dm.FS)
        for name, mine in (("trace", r.channel), ("start", r.start_col), ("stop", r.stop_col), ("peak_col", r.peak_col), ("peak", r.peak)):
            assert mine.tobytes() == want[name].tobytes(), name
    # (the robust spread is the noise's alone, so 3 spreads is a low bar; at 12 and 2 the events are the bursts)
    assert dm.found(r.channel, r.peak_time, r.start_col, r.stop_col, ts, 1) == []
    # a quiet stretch of the first epoch: the statistics are those of its columns of the smoothed trace
    r = cwt.detect(dm.BAND, smooth=SMOOTH, baseline=(2.2, 2.9))
    assert r.baseline_cols == (2200, 2900)
    for ch in range(2):
        cnt, m, s = dm.model_stats(trace[ch, 2200:2900])
        bm, bs = dm.stats_bound(trace[ch, 2200:2900])
        assert r.n_columns[ch] == cnt == 700 and abs(r.mean[ch] - m) <= bm and abs(r.sd[ch] - s) <= bs
    assert np.array_equal(r.n_candidates, dm.model_runs(trace, r.lo)["counts"])


def test_the_stated_defaults_are_the_call_without_them(recorded):
    for stride in (1, 4):
        cwt = recorded[stride]
        a, b = cwt.detect(dm.BAND), cwt.detect(dm.BAND, smooth=None, combine=False)
        for name in ("channel", "start", "stop", "peak_time", "peak", "start_col", "stop_col", "peak_col", "mean", "sd", "lo", "hi",
                     "n_columns", "n_candidates"):
            assert getattr(a, name).dtype == getattr(b, name).dtype and getattr(a, name).tobytes() == getattr(b, name).tobytes(), name
        assert (a.smooth, a.half, a.combined) == (b.smooth, b.half, b.combined) == (None, 0, False)
        assert a.channel.tolist() == [0] * 4 + [1] * 4


# -- 7. side effects -------------------------------------------------------------------------------------------------------
def test_the_resident_result_and_the_device_memory_are_as_they_were(recorded, monkeypatch):
    from ghost_amd import _lib, engine
    cwt = recorded[1]
    before = cwt.fetch()
    lazy = cwt._pending
    first = cwt.detect(dm.BAND, smooth=SMOOTH, combine=True)                # (whatever the first call sets up once is set up)
    made = []

    class Tracked(engine.DeviceBuffer):
        def __init__(self, nbytes):
            super().__init__(nbytes)
            made.append(self)

    monkeypatch.setattr(engine, "DeviceBuffer", Tracked)
    free = engine.device_memory()[0]

    def settled(n_buffers):
        assert len(made) == n_buffers and not any(b.ptr for b in made), [b.nbytes for b in made if b.ptr]
        assert abs(engine.device_memory()[0] - free) < 1 << 20
        del made[:]

    again = cwt.detect(dm.BAND, smooth=SMOOTH, combine=True)
    settled(3)                                                              # the trace, the smoothed trace and the runs
    for name in ("channel", "start", "stop", "peak_time", "peak", "start_col", "stop_col", "peak_col", "mean", "sd", "lo", "hi"):
        assert np.asarray(getattr(first, name)).tobytes() == np.asarray(getattr(again, name)).tobytes(), name
    cwt.detect(dm.BAND, smooth=SMOOTH)
    settled(3)
    cwt.detect(dm.BAND)
    settled(2)                                                              # the defaults: the trace and the runs, as before
    # the band trace is freed as soon as it has been smoothed: by the statistics only the smoothed one is left
    real = engine.trace_stats

    def stats(*args):
        assert [bool(b.ptr) for b in made] == [False, True]
        return real(*args)

    monkeypatch.setattr(engine, "trace_stats", stats)
    cwt.detect(dm.BAND, smooth=SMOOTH)
    settled(3)
    monkeypatch.setattr(engine, "trace_stats", real)
    # the temporaries are freed when a step raises, in the smoother and after it
    monkeypatch.setattr(engine, "segments_of", lambda *a: np.array([[0, 10], [5, 20]]))
    for _ in range(8):
        with pytest.raises(_lib.GhostCwtError, match=r"gcwt_trace_smooth: segments\[1\]"):
            cwt.detect(dm.BAND, smooth=SMOOTH)
    settled(16)
    monkeypatch.undo()
    monkeypatch.setattr(engine, "DeviceBuffer", Tracked)
    for _ in range(8):
        with pytest.raises(ValueError, match="lo >= 0"):
            cwt.detect(dm.BAND, smooth=SMOOTH, combine=True, threshold=-40.0, edge=-50.0)
    settled(16)
    with pytest.raises(ValueError, match="'smooth'"):                      # a refusal: before any device work
        cwt.detect(dm.BAND, smooth=-1.0)
    settled(0)
    assert cwt._pending is lazy
    assert cwt.fetch().tobytes() == before.tobytes()
    assert len(cwt.detect(dm.BAND)) == 8
