"""triggered() on the MI355X (csrc/triggered.hip, include/ghostcwt.h: gcwt_triggered): the kernel against the float64
model of the definition on its own input (tests/triggered_model.py), end to end against the oracle, together with
output_stride / epochs / Morlet / the single-channel call / freq_limits, its order and side effects, its error surface,
and a shape that exercises the tiling.

The bounds are derived, not measured (triggered_model.amplitude_bound / power_bound / evoked_bound / vector_bound /
itpc_bound): the worst-case float32 rounding of the prescribed terms (2, 2, 0 and 4 roundings) and order -- a chain of
ceil(E / 4) adds, 2 for the combination of the four chains, the divide."""
import numpy as np
import pytest

import triggered_model as tm
from oracle import ghost_oracle as orc

pytestmark = pytest.mark.gpu

FS = 1000.0
NAMES = ("amplitude", "power", "evoked", "vector", "itpc")


def _resident(x, freqs, **kw):
    from ghost_amd.engine import CwtPlan
    x = np.atleast_2d(np.asarray(x, dtype=np.float32))
    plan = CwtPlan(x.shape[1], x.shape[0], FS, freqs, output="complex", **kw)
    return plan, plan.execute_resident(x)


def _run(result, cols, nb, na, rows=None):
    from ghost_amd import engine
    res = engine.triggered(result, np.asarray(cols, dtype=np.int64), nb, na, rows)
    try:
        assert (res.n_rows, res.n_lags, res.n_events) == (result.shape[1] if rows is None else rows[1], nb + na + 1, len(cols))
        return res.to_host()
    finally:
        res.free()


def _compare(got, ref, n_events, msg=""):
    """The device's five outputs against the model's (same shapes); returns the worst ratios to the bounds, in the order
    of NAMES."""
    for name in NAMES:
        assert got[name].shape == ref[name].shape, (msg, name, got[name].shape, ref[name].shape)
        assert got[name].dtype == (np.complex64 if name in ("evoked", "vector") else np.float32), (msg, name)
    amp = ref["amplitude"]
    live = amp > 0
    err = {"amplitude": np.abs(got["amplitude"] - amp)[live] / amp[live],
           "power": np.abs(got["power"] - ref["power"])[live] / ref["power"][live],
           "evoked": np.abs(got["evoked"] - ref["evoked"])[live] / amp[live],
           "vector": np.abs(got["vector"] - ref["vector"]).ravel(),
           "itpc": np.abs(got["itpc"] - ref["itpc"]).ravel()}
    bound = {"amplitude": tm.amplitude_bound(n_events), "power": tm.power_bound(n_events), "evoked": tm.evoked_bound(n_events),
             "vector": tm.vector_bound(n_events), "itpc": tm.itpc_bound(n_events)}
    worst = np.array([err[name].max(initial=0.0) / bound[name] for name in NAMES])
    print("%s E=%d: error / bound: %s" % (msg, n_events, ", ".join("%s %.3f" % (k, v) for k, v in zip(NAMES, worst))))
    for name, ratio in zip(NAMES, worst):
        assert ratio <= 1.0, (msg, name, n_events, ratio)
    assert got["itpc"].min() >= 0.0 and got["itpc"].max() <= 1.0, msg
    for name in NAMES:                                # cells without signal: exactly 0 in all five
        assert not np.any(got[name][~live]), (msg, name)
    return worst


def _rows_of(d, first, count):
    return {k: v[:, first:first + count] for k, v in d.items()}


def _events(n_events, nb, na, n, rng, extra=()):
    """Unsorted event columns: one at nb, one at n - 1 - na (the first and last whose window fits), one duplicate, two
    whose windows overlap, ``extra`` where there is room, the rest drawn."""
    lo, hi = nb, n - 1 - na
    ev = [lo, hi][:n_events]
    if n_events >= 3:
        ev.append(int(rng.integers(lo, hi + 1)))
    if n_events >= 4:
        ev.append(ev[2])                              # the duplicate
    if n_events >= 5:
        ev.append(min(hi, ev[2] + (nb + na) // 2 + 1))   # overlaps ev[2]'s window (or follows it directly when L = 1)
    for e in extra:
        if len(ev) < n_events and lo <= e <= hi:
            ev.append(e)
    while len(ev) < n_events:
        ev.append(int(rng.integers(lo, hi + 1)))
    ev = np.array(ev, dtype=np.int64)[rng.permutation(n_events)]
    if np.all(np.diff(ev) >= 0):
        ev = ev[::-1].copy()
    assert ev.size == n_events and (n_events < 2 or nb + na == 0 or np.any(np.diff(ev) < 0))
    return ev


WINDOWS = ((0, 0), (0, 1), (31, 32), (63, 0), (100, 163), (0, 300))
ROW_RUNS = ((0, 14), (3, 4), (12, 1), (5, 8))


# -- 1. the kernel against float64 NumPy on its own input -------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 3])
def test_kernel_meets_the_model_on_its_own_input(c):
    from ghost_amd.synthetic import lfp
    n = 5003
    x = lfp(c, n, FS, seed=11)
    kw = dict(epoch_bounds=[[0, 2000], [2700, n]]) if c == 3 else {}       # (a gap: columns that are exactly 0)
    plan, result = _resident(x, np.geomspace(200.0, 4.0, 14), **kw)
    assert result.pitch % 32 == 0 and result.pitch > n
    w = result.to_host(np.complex64)
    if c == 3:
        assert not np.any(w[..., 2000:2700]) and np.all(np.abs(w[..., 1990:2000]) > 0)
    rng = np.random.default_rng(17)
    worst = np.zeros(5)
    for nb, na in WINDOWS:
        for n_events in (1, 2, 3, 4, 5, 67):
            cols = _events(n_events, nb, na, n, rng, extra=(1995, 2705, 2350) if c == 3 else ())
            ref = tm.model(w, cols, nb, na)                                    # once: a row's cells do not depend on the run
            for first, count in ROW_RUNS:
                got = _run(result, cols, nb, na, (first, count))
                worst = np.maximum(worst, _compare(got, _rows_of(ref, first, count), n_events,
                                                   "C=%d (%d, %d) rows %s" % (c, nb, na, (first, count))))
    print("C=%d: worst error / bound: %s" % (c, ", ".join("%s %.3f" % (k, v) for k, v in zip(NAMES, worst))))
    if c == 3:
        for nb, na in WINDOWS:
            got = _run(result, [2350], nb, na)                                 # an event inside the gap alone: exactly 0
            for name in NAMES:
                assert got[name].shape == (3, 14, nb + na + 1) and not np.any(got[name]), (name, nb, na)
            cols = [1995, 2705, 2350] if (nb, na) != (0, 0) else [1999, 2000, 2699]
            got = _run(result, cols, nb, na)                                   # windows reaching into the gap add zeros
            ref = tm.model(w, cols, nb, na)
            _compare(got, ref, 3, "C=3 (%d, %d) at the gap" % (nb, na))
            if nb + na:
                assert np.all(got["amplitude"] > 0)
            else:                                                              # 1999 alone has signal: a third of it is left
                np.testing.assert_allclose(got["amplitude"][..., 0], np.abs(w[..., 1999]) / 3, rtol=1e-6)
                np.testing.assert_allclose(got["itpc"], 1.0 / 3, rtol=1e-6)
    result.free()
    plan.close()


# -- 2. end to end against the oracle ----------------------------------------------------------------------------------
def test_class_surface_meets_the_oracle_and_the_physics():
    from ghost_amd.wave import ContinuousWaveletTransform
    n = 32768
    x, events = tm.evoked_input(n, FS)
    cwt = ContinuousWaveletTransform()
    cwt.transform(x, fs=FS, multichannel=True, output="complex", freq_limits=[4, 200], voices_per_octave=4)
    f = cwt.frequencies
    np.testing.assert_allclose(f, orc.frequency_grid(FS, n, freq_limits=(4, 200), voices_per_octave=4), rtol=1e-13)
    got = cwt.triggered(events, before=0.2, after=0.4)
    nb, na, n_lags = 200, 400, 601
    for name in NAMES:
        assert getattr(got, name).shape == (2, 23, n_lags), name
        assert getattr(got, name).dtype == (np.complex64 if name in ("evoked", "vector") else np.float32), name
    np.testing.assert_allclose(got.lags, np.arange(-nb, na + 1) / FS, rtol=0, atol=1e-15)
    np.testing.assert_array_equal(got.frequencies, f)
    assert got.n_events == 60 and got.events_used.shape == (60,) and got.events_used.all()
    dev = {name: getattr(got, name) for name in NAMES}
    tm.check_physics(dev, f, nb, FS)
    # every cell against the oracle, within what the transform's own gate allows
    ref_w = np.stack([orc.cwt_complex(x[ch], FS, f) for ch in range(2)])
    cols = np.round(events * FS).astype(np.int64)
    ref = tm.model(ref_w, cols, nb, na)
    gate = tm.gate_bound(ref_w, cols, nb, na)
    largest = max(v.max() for v in gate.values())
    print("largest gate bound %.3g" % largest)
    assert largest <= 1e-2, largest
    rounding = {"amplitude": tm.amplitude_bound(60) * ref["amplitude"], "power": tm.power_bound(60) * ref["power"],
                "evoked": tm.evoked_bound(60) * ref["amplitude"], "vector": tm.vector_bound(60), "itpc": tm.itpc_bound(60)}
    for name in NAMES:
        err = np.abs(dev[name] - ref[name])
        bound = gate[name] + rounding[name]
        print("%s: max |dev - ref| %.3g, max gate bound %.3g, worst error / bound %.3f"
              % (name, err.max(), gate[name].max(), (err / bound).max()))
        assert np.all(err <= bound), (name, err.max(), (err / bound).max())


# -- 3. it composes with what exists -----------------------------------------------------------------------------------
def _as_dict(got):
    d = {name: getattr(got, name) for name in NAMES}
    return {k: v[None] for k, v in d.items()} if got.itpc.ndim == 2 else d


def test_composes_with_output_stride_epochs_morlet_the_single_channel_call_and_freq_limits(golden):
    from ghost_amd.engine import coupling_rows, trigger_columns
    from ghost_amd.synthetic import lfp
    from ghost_amd.wave import ContinuousWaveletTransform, Morlet
    n = 30001
    x = lfp(4, n, FS, seed=5)
    ts = 3.25 + np.arange(n) / FS
    rng = np.random.default_rng(9)
    # a strided result with offset timestamps: the model on the fetched strided coefficients; lags count columns of 4 / fs
    events = np.concatenate([3.25 + rng.uniform(0.0, 30.0, 40), [0.0, 3.3, 33.2, 40.0]])     # four that cannot be used
    cwt = ContinuousWaveletTransform()
    cwt.transform(x, timestamps=ts, fs=FS, freq_limits=[4, 250], multichannel=True, output="complex", output_stride=4,
                  dtype=np.float32)
    _ = cwt.time                                   # (asked for before: the stride must not be forgotten with it)
    got = cwt.triggered(events, before=0.1, after=0.25)
    cols, used, nb, na = trigger_columns(events, ts[::4], FS, 4, 0.1, 0.25)
    assert (nb, na) == (25, 62) and not used[-4:].any() and 30 <= cols.size <= 40
    np.testing.assert_array_equal(got.events_used, used)
    assert got.n_events == cols.size
    np.testing.assert_allclose(got.lags, np.arange(-25, 63) * 4 / FS, rtol=0, atol=1e-15)
    np.testing.assert_allclose(got.lags * FS / 4, np.rint(got.lags * FS / 4), rtol=0, atol=1e-9)
    w = cwt.fetch(dtype=np.float32)
    assert w.shape == (4, cwt.frequencies.size, -(-n // 4)) and w.dtype == np.complex64
    assert got.itpc.shape == (4, cwt.frequencies.size, 88)
    np.testing.assert_array_equal(got.frequencies, cwt.frequencies)
    _compare(_as_dict(got), tm.model(w, cols, nb, na), cols.size, "stride 4")

    # G5's recording in two epochs (a gap in time) through the class surface: what would cross the gap is dropped
    g = golden("g5_two_epochs.npz")
    xs = np.stack([g["x"], g["x"][::-1]])
    gts = np.asarray(g["timestamps"])
    assert gts[5999] == 5.999 and gts[6000] == 16.0
    cwt = ContinuousWaveletTransform()
    cwt.transform(xs, fs=float(g["fs"]), timestamps=gts, multichannel=True, output="complex", dtype=np.float32)
    events = [1.0, 5.0, 5.95, 10.0, 16.02, 16.05, 18.0, 5.899, 19.9, 0.04, 17.5]
    got = cwt.triggered(events, before=0.05, after=0.1)
    #                                   in     in   crosses  gap   crosses  fits    in   fits  leaves  leaves  in
    assert got.events_used.tolist() == [True, True, False, False, False, True, True, True, False, False, True]
    cols = np.array([1000, 5000, 6050, 8000, 5899, 7500])
    assert got.n_events == 6 and got.amplitude.shape == (2, cwt.frequencies.size, 151)
    _compare(_as_dict(got), tm.model(cwt.fetch(dtype=np.float32), cols, 50, 100), 6, "G5")

    # a Morlet transform
    cwt = ContinuousWaveletTransform(wavelet=Morlet(w0=6))
    cwt.transform(x[:3, :20000], fs=FS, freq_limits=[5, 200], voices_per_octave=4, multichannel=True, output="complex",
                  dtype=np.float32)
    events = rng.uniform(0.5, 19.0, 33)
    got = cwt.triggered(events, before=0.3, after=0.3)
    assert got.events_used.all() and got.vector.shape == (3, cwt.frequencies.size, 601)
    _compare(_as_dict(got), tm.model(cwt.fetch(dtype=np.float32), np.rint(events * FS).astype(np.int64), 300, 300), 33, "Morlet")
    # ... and a band of it
    band = cwt.triggered(events, before=0.3, after=0.3, freq_limits=(20, 100))
    first, count = coupling_rows((20, 100), cwt.frequencies, "freq_limits")
    assert 1 < count < cwt.frequencies.size and first > 0
    np.testing.assert_array_equal(band.frequencies, cwt.frequencies[first:first + count])
    assert band.frequencies.min() >= 20 and band.frequencies.max() <= 100
    for name in NAMES:
        np.testing.assert_array_equal(getattr(band, name), getattr(got, name)[:, first:first + count], err_msg=name)

    # the reference's single-channel call: the channel axis is dropped; ascending freqs=
    cwt = ContinuousWaveletTransform()
    cwt.transform(x[1, :20000], fs=FS, freqs=[6.0, 8.0, 10.0, 60.0, 80.0, 100.0, 120.0], output="complex", dtype=np.float32)
    got = cwt.triggered(events, before=0.0, after=0.5, freq_limits=(8, 100))
    assert got.itpc.shape == (5, 501) and got.evoked.shape == (5, 501) and got.evoked.dtype == np.complex64
    np.testing.assert_array_equal(got.frequencies, [8.0, 10.0, 60.0, 80.0, 100.0])
    assert got.lags[0] == 0.0 and got.lags[-1] == 0.5
    w = cwt.fetch(dtype=np.float32)
    assert w.shape == (7, 20000)
    _compare(_as_dict(got), tm.model(w[None], np.rint(events * FS).astype(np.int64), 0, 500, (1, 5)), 33, "single channel")


# -- 4. order, determinism and side effects ----------------------------------------------------------------------------
def test_order_determinism_and_side_effects():
    from ghost_amd.synthetic import lfp
    from ghost_amd.wave import ContinuousWaveletTransform
    n, c = 20011, 3
    x = lfp(c, n, FS, seed=3)
    plan, result = _resident(x, np.geomspace(150.0, 5.0, 24))
    rng = np.random.default_rng(4)
    for n_events in (3, 150):
        cols = rng.integers(300, n - 300, n_events)
        a, b = _run(result, cols, 100, 163, (2, 19)), _run(result, cols, 100, 163, (2, 19))   # tiles of 4 rows: 4 x 4 + 3
        for name in NAMES:
            np.testing.assert_array_equal(a[name], b[name], err_msg=name)
        # a row alone -- inside a tile, the first of one, in the ragged last tile -- is the row inside the run, bit for bit
        for r in (0, 1, 3, 4, 11, 16, 18):
            alone = _run(result, cols, 100, 163, (2 + r, 1))
            for name in NAMES:
                np.testing.assert_array_equal(alone[name][:, 0], a[name][:, r], err_msg="%s row %d" % (name, r))
        # ... and inside a run that starts elsewhere, so that the row sits in another place of another tile
        other = _run(result, cols, 100, 163, (5, 19))
        for name in NAMES:
            np.testing.assert_array_equal(other[name][:, 0:16], a[name][:, 3:19], err_msg=name)
        # the same absolute lags inside another (nb, na): other lanes of other tiles, the same bits
        shifted = _run(result, cols, 37, 200, (2, 19))
        for name in NAMES:
            np.testing.assert_array_equal(shifted[name][..., 0:201], a[name][..., 63:264], err_msg=name)
        if n_events > 4:                             # (the order given is part of the definition: this is no accident)
            again = _run(result, cols[::-1].copy(), 100, 163, (2, 19))
            np.testing.assert_allclose(again["power"], a["power"], rtol=tm.power_bound(n_events) * 2)
    result.free()
    plan.close()

    # the resident result and the pending lazy fetch are as they were
    kw = dict(fs=FS, freq_limits=[5, 200], voices_per_octave=4, multichannel=True, output="complex")
    events = rng.uniform(0.5, 8.5, 25)
    one, twin = ContinuousWaveletTransform(), ContinuousWaveletTransform()
    one.transform(x[:3, :9000], **kw)
    twin.transform(x[:3, :9000], **kw)
    first = one.triggered(events, before=0.2, after=0.2)
    np.testing.assert_array_equal(one.fetch(slice(1, 4), 100, 5000), twin.fetch(slice(1, 4), 100, 5000))
    assert one._pending is not None                  # still lazy: nothing was brought over
    np.testing.assert_array_equal(one.coefficients, twin.coefficients)
    assert one.coefficients.dtype == np.complex128
    again = one.triggered(events, before=0.2, after=0.2)                     # ... and after the result has been brought over
    for name in NAMES:
        np.testing.assert_array_equal(getattr(first, name), getattr(again, name), err_msg=name)
    np.testing.assert_array_equal(one.fetch(), twin.fetch())


# -- 5. the error surface on the device --------------------------------------------------------------------------------
def test_error_surface_on_the_device():
    from ghost_amd.synthetic import lfp
    from ghost_amd.wave import ContinuousWaveletTransform
    x = lfp(4, 8192, FS, seed=1)
    kw = dict(fs=FS, freq_limits=[8, 200], voices_per_octave=4)
    events = [1.0, 2.5, 4.0, 7.0]
    cwt = ContinuousWaveletTransform()
    cwt.transform(x, multichannel=True, **kw)                                     # amplitude
    with pytest.raises(ValueError, match="complex"):
        cwt.triggered(events, before=0.1, after=0.1)
    cwt = ContinuousWaveletTransform()
    cwt.transform(x, multichannel=True, output="complex", devices=[0, 0], **kw)   # sharded
    with pytest.raises(ValueError, match="devices"):
        cwt.triggered(events, before=0.1, after=0.1)
    cwt = ContinuousWaveletTransform()
    cwt.transform(x, multichannel=True, output="complex", **kw)
    with pytest.raises(ValueError, match="none of the 3 events") as info:
        cwt.triggered([0.05, 8.15, 20.0], before=0.1, after=0.1)                  # no event survives: how many and why
    assert "1 lie in a gap" in str(info.value) and "2 have a window" in str(info.value)
    with pytest.raises(ValueError, match="none of the 0 events"):
        cwt.triggered([], before=0.1, after=0.1)
    with pytest.raises(ValueError, match="before"):
        cwt.triggered(events, before=-0.1, after=0.1)
    with pytest.raises(ValueError, match="before"):
        cwt.triggered(events, before=np.nan, after=0.1)
    with pytest.raises(ValueError, match="after"):
        cwt.triggered(events, before=0.1, after=np.inf)
    with pytest.raises(ValueError, match="events"):
        cwt.triggered([1.0, np.nan], before=0.1, after=0.1)
    with pytest.raises(ValueError, match="freq_limits"):
        cwt.triggered(events, before=0.1, after=0.1, freq_limits=(1, 4))          # a band with no rows
    with pytest.raises(TypeError):
        cwt.triggered(events, 0.1, after=0.1)                                     # positional before
    with pytest.raises(TypeError):
        cwt.triggered(events, 0.1, 0.1)
    with pytest.raises(TypeError):
        cwt.triggered(events, after=0.1)
    got = cwt.triggered(events, before=0.1, after=0.1)
    assert got.itpc.shape == (4, cwt.frequencies.size, 201) and got.n_events == 4 and got.events_used.all()
    assert np.all(got.amplitude > 0) and np.all(got.itpc <= 1)


# -- 6. a shape that exercises the tiles -------------------------------------------------------------------------------
def test_sixteen_channels_forty_rows_a_thousand_lags():
    from ghost_amd.synthetic import lfp
    c, n, n_events, nb, na = 16, 1 << 18, 500, 300, 700
    x = lfp(c, n, FS, seed=21)
    plan, result = _resident(x, np.geomspace(200.0, 2.0, 40))
    rng = np.random.default_rng(6)
    cols = rng.integers(nb, n - na, n_events)
    got = _run(result, cols, nb, na)
    n_lags = nb + na + 1
    for name in NAMES:
        assert got[name].shape == (16, 40, n_lags), name
    assert got["itpc"].min() >= 0.0 and got["itpc"].max() <= 1.0
    cells = [(int(rng.integers(16)), int(rng.integers(40)), int(rng.integers(n_lags))) for _ in range(200)]
    cells += [(0, 0, 0), (0, 0, n_lags - 1), (15, 39, 0), (15, 39, n_lags - 1)]                 # the corners
    bound = {"amplitude": tm.amplitude_bound(n_events), "power": tm.power_bound(n_events), "evoked": tm.evoked_bound(n_events),
             "vector": tm.vector_bound(n_events), "itpc": tm.itpc_bound(n_events)}
    worst = dict.fromkeys(NAMES, 0.0)
    for ch, r, lag in cells:
        # the row of this cell alone, straight from the device; the cell is lag 0 of the events moved by its lag
        row = result.buffer.download((n,), np.complex64, ((ch * 40 + r) * result.pitch) * 8)
        ref = tm.model(row[None, None], cols - nb + lag, 0, 0)
        amp = ref["amplitude"][0, 0, 0]
        for name in NAMES:
            err = abs(got[name][ch, r, lag] - ref[name][0, 0, 0])
            scale = {"amplitude": amp, "power": ref["power"][0, 0, 0], "evoked": amp}.get(name, 1.0)
            worst[name] = max(worst[name], err / scale / bound[name])
            assert err <= bound[name] * scale, (ch, r, lag, name, err, bound[name] * scale)
    print("16 channels, 40 rows, %d lags, %d events: worst error / bound: %s"
          % (n_lags, n_events, ", ".join("%s %.3f" % kv for kv in worst.items())))
    result.free()
    plan.close()
