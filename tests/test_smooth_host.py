"""detect(smooth=, combine=) without a GPU: the NumPy model of gcwt_trace_smooth against SciPy's Gaussian filter run per
segment, engine.smooth_taps and engine.segments_of, the C entry's argument checks (they come before any device call), the
refusals of the method, and the estimator -- smoothed and combined -- on the oracle's coefficients.  The device side:
tests/test_gpu_smooth.py."""
import ctypes as C

import numpy as np
import pytest

import detect_model as dm
import smooth_model as sm

FS = 1000.0


# -- the model ------------------------------------------------------------------------------------------------------------
def test_the_model_is_scipys_gaussian_filter_run_per_segment():
    """gaussian_filter1d(mode='constant') takes float64 weights; the model takes them rounded to float32: each differs by at
    most u w_k, so the two results by at most u sum_k w_k (|v[c - k]| + |v[c + k]|), plus float64 rounding of either sum."""
    from scipy.ndimage import gaussian_filter1d
    rng = np.random.default_rng(0)
    n = 700
    v = (rng.standard_normal(n) * 3 + 1).astype(np.float32)
    segments = np.array([[0, 1], [1, 9], [9, 300], [340, 341], [350, n - 2]])
    for sd in (0.125, 0.3, 1.0, 4.0, 7.3, 40.0):
        w = sm.taps(sd)
        assert len(w) - 1 == int(4 * sd + 0.5)
        got = sm.smooth(v, w, segments)
        want = np.zeros(n)
        for a, b in segments:
            want[a:b] = gaussian_filter1d(v[a:b].astype(np.float64), sd, mode="constant", truncate=4.0)
        room = (sm.U + 64 * len(w) * sm.U64) * sm.bound(v, w, segments) / sm.gamma(len(w))
        assert np.all(np.abs(got - want) <= room), (sd, np.abs(got - want).max(), room.max())
        assert not got[1 - 1 + 300:340].any() and not got[341:350].any() and not got[n - 2:].any()
    # one segment: the whole trace
    w = sm.taps(2.0)
    assert np.allclose(sm.smooth(v, w), gaussian_filter1d(v.astype(np.float64), 2.0, mode="constant"), rtol=0, atol=1e-5)


def test_model_combine_is_the_float32_chain():
    rng = np.random.default_rng(1)
    t = (rng.standard_normal((5, 40)) * 1e3).astype(np.float32)
    got = sm.combine(t, [3, 0, 3, 4])
    for c in range(40):
        s = np.float32(t[3, c])
        for m in (0, 3, 4):
            s = np.float32(s + t[m, c])
        assert got[c] == np.float32(s * np.float32(0.25))
    assert sm.combine(t, [2]).tobytes() == t[2].tobytes()
    third = sm.combine(t, [0, 1, 2])
    assert third.dtype == np.float32 and np.float32(1.0 / 3) == np.float32(0.333333343267)
    assert not np.array_equal(sm.combine(t, [0, 1, 2, 3, 4]), sm.combine(t, [4, 3, 2, 1, 0]))      # the order is part of it


def test_model_bound_holds_for_the_float32_chain():
    """The prescribed chain, run in NumPy float32 (a fused multiply-add made from float64, exact for float32 operands), stays
    inside the derived bound around the float64 model."""
    rng = np.random.default_rng(2)
    n = 300
    v = (rng.standard_normal(n) + 5).astype(np.float32)
    segments = np.array([[0, 120], [120, 127], [150, n]])
    for half in (0, 1, 3, 16, 65, 200):
        w = sm.taps_of_half(half)
        want, room = sm.smooth(v, w, segments), sm.bound(v, w, segments)
        got = np.zeros(n, np.float32)
        for a, b in segments:
            for c in range(a, b):
                acc = np.float32(w[0] * v[c])
                for k in range(1, half + 1):
                    pair = np.float32((v[c - k] if c - k >= a else np.float32(0)) + (v[c + k] if c + k < b else np.float32(0)))
                    acc = np.float32(np.float64(w[k]) * np.float64(pair) + np.float64(acc))   # 24 x 24 bits: the product is exact
                got[c] = acc
        assert np.all(np.abs(got - want) <= room), (half, np.abs(got - want).max())
        assert room.max() < 1e-4 * (half + 1)


# -- engine.smooth_taps, engine.segments_of ---------------------------------------------------------------------------------
def test_smooth_taps():
    from ghost_amd import _lib, engine
    assert _lib.SMOOTH_MAX_HALF == 4096
    for sd, half in ((0.125, 1), (0.3749, 1), (0.375, 2), (1.0, 4), (4.0, 16), (16.0, 64), (120.0, 480), (1024.0, 4096)):
        w = engine.smooth_taps(sd)
        assert w.dtype == np.float32 and w.shape == (half + 1,), sd
        assert w.tobytes() == sm.taps(sd).tobytes()
        total = float(w[0].astype(np.float64) + 2 * w[1:].astype(np.float64).sum())
        assert abs(total - 1) <= 2 * sm.U * (half + 1), (sd, total - 1)
        assert np.all(w > 0) and np.all(np.diff(w) < 0)
    with pytest.raises(ValueError, match="narrower than a column"):
        engine.smooth_taps(0.124)
    with pytest.raises(ValueError, match="above the limit of 4096.*output_stride"):
        engine.smooth_taps(1024.2)
    with pytest.raises(ValueError, match="above the limit"):
        engine.smooth_taps(1e300)
    for bad in (0, -1.0, np.nan, np.inf, "4", None, True, [4.0]):
        with pytest.raises(ValueError, match="'sd_cols'"):
            engine.smooth_taps(bad)


def test_segments_of_is_trigger_columns_splice_rule():
    """A window of one column before an event at column j is refused as a splice exactly where a segment begins at j."""
    from ghost_amd import engine
    _, ts = dm.recording()
    for stride in (1, 4):
        t, period = ts[::stride], stride / dm.FS
        n = t.size
        got = engine.segments_of(t, period, dm.FS, n)
        assert got.dtype == np.int64 and got.tolist() == [[0, dm.SPLIT // stride], [dm.SPLIT // stride, n]]
        assert got.tolist() == sm.segments_of(t, period, dm.FS, n).tolist()
        _, used, nb, na = engine.trigger_columns(t[1:], t, dm.FS, stride, period, 0.0)
        assert (nb, na) == (1, 0)
        assert (np.flatnonzero(~used) + 1).tolist() == got[1:, 0].tolist()
        # fewer columns than times; no clock at all
        assert engine.segments_of(t, period, dm.FS, 100).tolist() == [[0, 100]]
        assert engine.segments_of(None, period, dm.FS, n).tolist() == [[0, n]]
    # jitter below half a sample is no boundary, more is; a step back is one too
    t = np.arange(10) / FS
    t[4:] += 0.4 / FS
    assert engine.segments_of(t, 1 / FS, FS, 10).tolist() == [[0, 10]]
    t[7:] += 0.2 / FS
    t[4:] += 0.2 / FS
    assert engine.segments_of(t, 1 / FS, FS, 10).tolist() == [[0, 4], [4, 10]]
    t[9] = t[2]
    assert engine.segments_of(t, 1 / FS, FS, 10).tolist() == [[0, 4], [4, 9], [9, 10]]
    with pytest.raises(ValueError, match="fewer"):
        engine.segments_of(t, 1 / FS, FS, 11)
    with pytest.raises(ValueError, match="at least one column"):
        engine.segments_of(None, 1 / FS, FS, 0)


# -- the C entry: arguments first, then the device ------------------------------------------------------------------------
def test_entry_point_validates_then_needs_a_device():
    from ghost_amd import _lib
    from ghost_amd.engine import device_count
    lib = _lib.lib
    buf, out = (C.c_float * 256)(), (C.c_float * 256)()
    w3 = (C.c_float * 3)(0.5, 0.2, 0.05)

    def i64(*v):
        return (C.c_int64 * len(v))(*v)

    def i32(*v):
        return (C.c_int32 * len(v))(*v)

    def call(trace=buf, pitch=64, c=4, n=60, taps=w3, half=2, seg=None, n_seg=0, mem=None, n_mem=0, out=out, out_pitch=64):
        return lib.gcwt_trace_smooth(trace, pitch, c, n, taps, half, seg, n_seg, mem, n_mem, out, out_pitch)

    long_taps = (C.c_float * 4098)(*([1e-4] * 4098))
    inside = C.cast(C.addressof(buf) + 4 * 100, C.POINTER(C.c_float))       # begins inside the traces
    behind = C.cast(C.addressof(buf) + 4 * (3 * 64 + 59), C.POINTER(C.c_float))   # begins on their last live column
    cases = (
        (dict(trace=None), b"d_trace is NULL"), (dict(c=0), b"n_traces"), (dict(n=0), b"n_cols"), (dict(pitch=59), b"pitch"),
        (dict(c=2**31, n=1), b"workgroups"),
        (dict(taps=None), b"taps is NULL"), (dict(half=-1), b"half"),
        (dict(taps=long_taps, half=4097), b"GCWT_SMOOTH_MAX_HALF = 4096"), (dict(taps=long_taps, half=4097), b"output_stride"),
        (dict(taps=(C.c_float * 3)(0.5, float("nan"), 0.1)), b"taps[1]"), (dict(taps=(C.c_float * 3)(float("inf"), 0.1, 0.1)), b"taps[0]"),
        (dict(taps=(C.c_float * 3)(0.5, 0.1, float("-inf"))), b"taps[2]"),
        (dict(seg=i64(0, 10), n_seg=0), b"together"), (dict(seg=None, n_seg=1), b"together"), (dict(seg=i64(0, 10), n_seg=-1), b"together"),
        (dict(seg=i64(0, 10, 9, 20), n_seg=2), b"segments[1] = [9, 20)"),                # overlapping
        (dict(seg=i64(0, 10, 30, 40, 12, 20), n_seg=3), b"segments[2] = [12, 20)"),      # unsorted
        (dict(seg=i64(0, 10, 12, 61), n_seg=2), b"segments[1] = [12, 61)"),              # past n_cols
        (dict(seg=i64(-1, 10), n_seg=1), b"segments[0] = [-1, 10)"),
        (dict(seg=i64(0, 10, 15, 15), n_seg=2), b"segments[1] = [15, 15)"),              # holds no column
        (dict(seg=i64(0, 10, 20, 15), n_seg=2), b"segments[1] = [20, 15)"),
        (dict(mem=i32(0, 1), n_mem=0), b"together"), (dict(mem=None, n_mem=2), b"together"),
        (dict(mem=i32(0, 4, 1), n_mem=3), b"members[1] = 4"), (dict(mem=i32(0, 1, -1), n_mem=3), b"members[2] = -1"),
        (dict(out=None), b"d_out is NULL"), (dict(out_pitch=59), b"out_pitch"),
        (dict(out=buf), b"overlaps"), (dict(out=inside), b"overlaps"), (dict(out=behind), b"overlaps"),
        (dict(out=inside, mem=i32(1, 2), n_mem=2), b"overlaps"),
    )
    for kw, word in cases:
        assert call(**kw) == _lib.ERR_INVALID, kw
        msg = lib.gcwt_last_error()
        assert msg.startswith(b"gcwt_trace_smooth:") and word in msg, (kw, msg)
    # valid requests: without a GPU there is nothing that computes them; with one, host memory is not a trace on a device
    n_dev = device_count()
    ahead = C.cast(C.addressof(buf) + 4 * (3 * 64 + 60), C.POINTER(C.c_float))    # the first byte behind the traces: no overlap
    for kw in (dict(), dict(half=0), dict(taps=long_taps, half=4096), dict(seg=i64(0, 10, 10, 11, 59, 60), n_seg=3),
               dict(mem=i32(3, 3, 0), n_mem=3), dict(pitch=60, out_pitch=60), dict(c=1, n=1), dict(out=ahead, mem=i32(0), n_mem=1)):
        rc = call(**kw)
        if n_dev == 0:
            assert rc == _lib.ERR_NO_DEVICE and b"no CPU path" in lib.gcwt_last_error(), kw
        else:
            assert rc == _lib.ERR_INVALID and b"device memory" in lib.gcwt_last_error(), kw


def test_engine_wrapper_refuses_before_the_library():
    from ghost_amd import engine
    w = sm.taps(1.0)
    with pytest.raises(ValueError, match="freed"):
        engine.trace_smooth(C.c_void_p(), 64, 1, 60, w)
    with pytest.raises(ValueError, match="n_cols"):
        engine.trace_smooth(4096, 64, 1, 60.0, w)
    for bad in (0.5, [[0.5, 0.2]], [], [True], ["a"]):
        with pytest.raises(ValueError, match="'taps'"):
            engine.trace_smooth(4096, 64, 1, 60, bad)
    for bad in ([0, 60], [[0, 30, 60]], [[0.0, 60.0]], np.zeros((0, 2), np.int64)):
        with pytest.raises(ValueError, match="'segments'"):
            engine.trace_smooth(4096, 64, 1, 60, w, segments=bad)
    for bad in (0, [], [[0]], [0.0], [True], [2], [-1]):
        with pytest.raises(ValueError, match="'members'"):
            engine.trace_smooth(4096, 64, 2, 60, w, members=bad)


# -- detect(): refusals that need no device --------------------------------------------------------------------------------
def test_detect_refuses_smooth_and_combine_it_cannot_use():
    from ghost_amd import engine
    from ghost_amd.wave import ContinuousWaveletTransform
    cwt = ContinuousWaveletTransform()
    cwt._frequencies, cwt._fs = np.geomspace(100.0, 10.0, 3), FS
    # a stub whose buffer no device call could survive: every refusal comes before the first one
    cwt._device_result, cwt._pending = engine.DeviceResult(object(), (2, 3, 100), 128, True), ("complex", np.float32, False)
    for bad in (-0.004, -1, 0, 0.0, np.nan, np.inf, "0.004", True, (0.004,)):
        with pytest.raises(ValueError, match=r"detect\(\): 'smooth' must be None or a finite number of seconds > 0"):
            cwt.detect((10.0, 100.0), smooth=bad)
    with pytest.raises(ValueError, match=r"detect\(\): 'smooth' = 0.0001 s.*narrower than a column"):
        cwt.detect((10.0, 100.0), smooth=0.0001)                                       # 0.1 columns: half = 0
    with pytest.raises(ValueError, match=r"detect\(\): 'smooth' = 1.1 s.*above the limit of 4096.*output_stride"):
        cwt.detect((10.0, 100.0), smooth=1.1)                                          # 4400 columns to either side
    cwt._stride = 8
    with pytest.raises(ValueError, match="narrower than a column"):
        cwt.detect((10.0, 100.0), smooth=0.0009)                                       # 0.1125 columns of 8 samples
    cwt._stride = 1
    for bad in (1, 0, None, "yes", [True]):
        with pytest.raises(ValueError, match=r"detect\(\): 'combine' must be True or False"):
            cwt.detect((10.0, 100.0), combine=bad)
    # the other refusals still come first or after, device untouched: a valid smooth with a bad threshold
    with pytest.raises(ValueError, match="hi < lo"):
        cwt.detect((10.0, 100.0), smooth=0.004, combine=True, threshold=1.0, edge=2.0)
    cwt._device_result, cwt._pending = engine.DeviceResult(object(), (1, 3, 100), 128, True), ("complex", np.float32, True)
    with pytest.raises(ValueError, match=r"detect\(\): 'combine'.*single-channel"):
        cwt.detect((10.0, 100.0), combine=True)
    with pytest.raises(ValueError, match=r"detect\(\): 'combine'.*single-channel"):
        cwt.detect((10.0, 100.0), combine=True, smooth=0.004)
    cwt._device_result = None


# -- the estimator on the oracle's coefficients: what the end-to-end test then asks of the device ---------------------------
def test_the_smoothed_model_finds_the_bursts_on_the_oracles_coefficients():
    """tests/test_gpu_smooth.py asks that detect(smooth=0.004) find every burst of detect_model.recording() exactly once,
    channel by channel and on the mean trace.  That the definition itself does -- on the oracle's float64 coefficients, for
    the envelope and the power, at every column and at every fourth -- is settled here, so that the condition there tests
    the device and not the estimator."""
    import bandpass_model as bm
    from ghost_amd import engine
    from ghost_amd.wave import Morse
    from oracle import ghost_oracle as orc
    x, ts = dm.recording()
    f = 250.0 / 2 ** (np.arange(6) / 4)                                     # freq_limits=[100, 250] at 4 voices per octave
    rows = engine.band_rows(dm.BAND, f)
    g, h = engine.band_weights(f, Morse(fs=dm.FS))
    epochs = np.array([[0, dm.SPLIT], [dm.SPLIT, dm.N]])
    w = np.stack([orc.cwt_complex(x[ch], dm.FS, f, epoch_bounds=epochs) for ch in range(2)])
    ref = bm.model(w, rows, g, h)
    everything = {-1: tuple(sorted(dm.BURSTS[0] + dm.BURSTS[1]))}
    seen = {}
    for on in ("envelope", "power"):
        for stride in (1, 4):
            raw, t = ref[on][:, 0, ::stride].astype(np.float32), ts[::stride]
            taps = engine.smooth_taps(0.004 * dm.FS / stride)
            segments = engine.segments_of(t, stride / dm.FS, dm.FS, t.size)
            for combined in (False, True):
                base = sm.combine(raw, [0, 1])[None] if combined else raw
                trace = np.stack([sm.smooth(v, taps, segments) for v in base]).astype(np.float32)
                counts = []
                for tr in (base, trace):                                    # unsmoothed, smoothed
                    stats = [dm.model_stats(v) for v in tr]
                    mean, sd = np.array([s[1] for s in stats]), np.array([s[2] for s in stats])
                    hi, lo = (mean + 3.0 * sd).astype(np.float32), mean.astype(np.float32)
                    runs = dm.model_runs(tr, lo)
                    counts.append(int(runs["counts"].sum()))
                ev = dm.model_events(runs, hi, t, 0.0, 0.0, None, stride / dm.FS)
                channel = np.full_like(ev["trace"], -1) if combined else ev["trace"]
                bursts = everything if combined else dm.BURSTS
                assert dm.found(channel, t[ev["peak_col"]], ev["start"], ev["stop"], ts, stride, bursts) == [], (on, stride, combined)
                assert len(ev["trace"]) == 8
                margin = float((ev["peak"] / hi[ev["trace"]]).min())
                assert margin > (1.25 if combined else 1.8), (on, stride, combined, margin)
                # smoothing removes candidates -- except from the mean power trace, whose only runs above its mean are the 8
                # bursts already: there is nothing to remove
                if (on, combined) == ("power", True):
                    assert counts == [8, 8], (stride, counts)
                else:
                    assert counts[1] < counts[0], (on, stride, combined, counts)
                seen[on, stride, combined] = (counts[0], counts[1], round(margin, 2))
    print(seen)
    assert seen["envelope", 1, False][:2] == (354, 224)
