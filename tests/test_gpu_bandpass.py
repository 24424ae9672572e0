"""bandpass() on the MI355X (csrc/bandpass.hip, include/ghostcwt.h: gcwt_bandpass): the kernel against the float64 model
of the definition on its own input (tests/bandpass_model.py) and, bit for bit, against the prescribed float32 chains; the
same bits whatever else is asked for; end to end against the oracle; the physical reading; together with output_stride /
freqs= / the single-channel call; its side effects.

The bounds are derived, not measured (bandpass_model.analytic_bound / envelope_extra / power_bound): a chain of R fused
multiply-adds along the R rows of a band, 2 more roundings in every term of the power, 2 for the modulus."""
import ctypes as C

import numpy as np
import pytest

import bandpass_model as bm
from oracle import ghost_oracle as orc

pytestmark = pytest.mark.gpu

FS = 1000.0
NAMES = ("analytic", "envelope", "power")
S = 23
T, G = 512, 4                                       # GCWT_BANDPASS_TILE_COLS, GCWT_BANDPASS_GROUP_BANDS

BAND_LISTS = {
    "all rows": [(0, S)],
    "one row": [(7, 1)],
    "first and last row": [(0, 1), (S - 1, 1)],
    "three overlapping runs": [(2, 9), (5, 9), (8, 12)],
    "G bands": [(k, 5) for k in range(G)],
    "G + 1 bands": [(3 * k, 6 + k) for k in range(G + 1)],
    "runs around the depth": [(1, 1), (2, 2), (3, 3), (4, 4), (5, 5), (6, 7), (7, 8), (8, 9), (3, 17)],
}


def _pitch(n):
    from ghost_amd.engine import _pitch
    return _pitch(n)


def _rows(c, n, seed):
    """(C, S, n) complex64 rows with a run of exactly-zero columns (where there is room), and weights: g of both signs."""
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((c, S, n)) + 1j * rng.standard_normal((c, S, n))).astype(np.complex64)
    if n >= 5:
        w[..., n // 3:n // 3 + max(1, n // 5)] = 0
    g = rng.standard_normal(S).astype(np.float32)
    assert g.min() < 0 < g.max()
    return w, g, rng.random(S).astype(np.float32)


def _upload(w, pitch):
    """The rows on the device as a resident result; what lies between n_cols and pitch is NaN: read perhaps, never used."""
    from ghost_amd.engine import DeviceBuffer, DeviceResult
    c, s, n = w.shape
    padded = np.full((c, s, pitch), np.nan + 1j * np.nan, np.complex64)
    padded[..., :n] = w
    buf = DeviceBuffer(padded.nbytes)
    buf.upload(padded)
    return DeviceResult(buf, (c, s, n), pitch, True)


def _run(result, bands, g, h, outputs=NAMES):
    from ghost_amd import engine
    res = engine.bandpass(result, np.asarray(bands, dtype=np.int32), g, h, outputs)
    try:
        assert (res.n_channels, res.n_bands, res.n_cols, res.outputs) == (result.shape[0], len(bands), result.shape[2], tuple(outputs))
        assert res.nbytes == sum(result.shape[0] * len(bands) * res.pitch * (8 if k == "analytic" else 4) for k in outputs)
        out = res.to_host()
    finally:
        res.free()
    assert tuple(out) == tuple(k for k in NAMES if k in outputs)
    return out


def _compare(got, w, bands, g, h, msg, gate=None):
    """The device's outputs against the float64 model on w: the worst error / bound of each (dtypes, shapes and exact
    zeros on the way)."""
    ref, t = bm.model(w, bands, g, h), bm.band_terms(w, bands, g)
    zero = ~np.any(np.asarray(w) != 0, axis=1)                              # C, n: the columns without signal
    worst = {}
    for name in got:
        assert got[name].shape == ref[name].shape and got[name].dtype == (np.complex64 if name == "analytic" else np.float32), (msg, name)
        assert not np.any(got[name][np.broadcast_to(zero[:, None], got[name].shape)]), (msg, name)
        err = np.abs(got[name] - ref[name])
        ratio = 0.0
        for k, (_, n) in enumerate(bands):
            bound = {"analytic": bm.analytic_bound(n) * t[:, k],
                     "envelope": bm.analytic_bound(n) * t[:, k] + bm.envelope_extra() * ref["envelope"][:, k],
                     "power": bm.power_bound(n) * ref["power"][:, k]}[name]
            if gate is not None:
                bound = bound + (gate[1][:, k] if name == "power" else gate[0][:, k])
            live = bound > 0
            assert not np.any(err[:, k][~live]), (msg, name, k)
            ratio = max(ratio, (err[:, k][live] / bound[live]).max(initial=0.0))
        worst[name] = ratio
    print("%s: error / bound: %s" % (msg, ", ".join("%s %.3f" % kv for kv in worst.items())))
    for name, ratio in worst.items():
        assert ratio <= 1.0, (msg, name, ratio)
    return worst


def _same_bits(a, b, msg):
    assert a.dtype == b.dtype and a.shape == b.shape, msg
    assert np.array_equal(a, b), (msg, int(np.count_nonzero(a != b)))


# -- 1. the kernel against float64 NumPy on its own input ----------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 3, 9])
def test_kernel_meets_the_model_on_its_own_input(c):
    worst = dict.fromkeys(NAMES, 0.0)
    for n, pitch in [(m, _pitch(m)) for m in (1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3)] + [(T + 32, T + 32)]:
        w, g, h = _rows(c, n, 100 * c + n)
        result = _upload(w, pitch)
        assert result.pitch % 32 == 0
        for what, bands in BAND_LISTS.items():
            msg = "C=%d n=%d %s" % (c, n, what)
            got = _run(result, bands, g, h)
            for name, ratio in _compare(got, w, bands, g, h, msg).items():
                worst[name] = max(worst[name], ratio)
            # the envelope is the prescribed modulus of the device's own analytic signal, bit for bit
            _same_bits(got["envelope"], np.sqrt(bm.norm2_32(got["analytic"])), msg)
            # ... and all three are the prescribed float32 chains, bit for bit
            chains = bm.chains32(w, bands, g, h)
            for name in NAMES:
                _same_bits(got[name], chains[name], msg + " " + name)
            if what in ("three overlapping runs", "G + 1 bands"):           # each output asked for alone: the same bits
                for name in NAMES:
                    alone = _run(result, bands, g if name != "power" else None, h if name == "power" else None, (name,))
                    _same_bits(alone[name], got[name], msg + " alone " + name)
        result.free()
    print("C=%d: worst error / bound: %s" % (c, ", ".join("%s %.3f" % kv for kv in worst.items())))


def test_rows_and_outputs_that_start_off_16_bytes():
    """The entry point takes any pitch >= n_cols: an odd one moves 8 bytes per column and gives the same bits; nothing is
    stored past n_cols."""
    from ghost_amd import _lib
    from ghost_amd.engine import DeviceBuffer
    c, n = 2, T + 7
    w, g, h = _rows(c, n, 77)
    bands = np.array(BAND_LISTS["G + 1 bands"], dtype=np.int32)
    aligned = _upload(w, _pitch(n))
    want = _run(aligned, bands, g, h)
    aligned.free()
    odd = _upload(w, n)
    out_pitch = n + 2
    planes = {"analytic": np.complex64, "envelope": np.float32, "power": np.float32}
    bufs = {}
    for name, dtype in planes.items():
        bufs[name] = DeviceBuffer(c * len(bands) * out_pitch * np.dtype(dtype).itemsize)
        bufs[name].upload(np.full((c, len(bands), out_pitch), 7.0, dtype))
    f32p = C.POINTER(C.c_float)
    _lib.check(_lib.lib.gcwt_bandpass(odd.buffer.ptr, n, c, S, n, bands.ctypes.data_as(C.POINTER(C.c_int32)), len(bands),
                                      g.ctypes.data_as(f32p), h.ctypes.data_as(f32p), bufs["analytic"].ptr, bufs["envelope"].ptr,
                                      bufs["power"].ptr, out_pitch))
    for name, dtype in planes.items():
        got = bufs[name].download((c, len(bands), out_pitch), dtype)
        _same_bits(np.ascontiguousarray(got[..., :n]), want[name], name)
        assert np.all(got[..., n:] == 7.0), name
        bufs[name].free()
    odd.free()


# -- 2. the same bits ------------------------------------------------------------------------------------------------------
def test_a_cell_has_the_same_bits_whatever_else_is_asked_for():
    c, n = 3, 2 * T + 3
    w, g, h = _rows(c, n, 5)
    result = _upload(w, _pitch(n))
    band = (4, 9)
    alone = _run(result, [band], g, h)
    others = [(0, S), (6, 3), (12, 11), (4, 8), (S - 1, 1)]
    for at in range(G + 1):                                                 # at every position of a list of G + 1
        bands = others[:G]
        bands.insert(at, band)
        got = _run(result, bands, g, h)
        for name in NAMES:
            _same_bits(np.ascontiguousarray(got[name][:, at:at + 1]), alone[name], "%s at %d" % (name, at))
    again = _run(result, [band], g, h)                                      # a second call
    for name in NAMES:
        _same_bits(again[name], alone[name], name)
    # the same buffer seen with fewer columns: other tiles are ragged, other lanes take the last column
    from ghost_amd.engine import DeviceResult
    full = _run(result, BAND_LISTS["three overlapping runs"], g, h)
    for m in (1, 2, T - 1, T, T + 1, 2 * T, 2 * T + 1, 2 * T + 2):
        view = DeviceResult(result.buffer, (c, S, m), result.pitch, True)
        got = _run(view, BAND_LISTS["three overlapping runs"], g, h)
        for name in NAMES:
            _same_bits(got[name], np.ascontiguousarray(full[name][..., :m]), "%s first %d columns" % (name, m))
    result.free()


# -- 3. end to end against the oracle ----------------------------------------------------------------------------------
def _meets_the_oracle(dev, x, f, rows, g, h, epochs, msg):
    """Every cell against the model on the oracle's float64 coefficients, within what the transform's own gate allows
    (bandpass_model.gate_bound) plus the rounding bound; the gap between the epochs is exactly 0."""
    n = x.shape[1]
    assert dev["analytic"].shape == (x.shape[0], len(rows), n)
    (_, gap_lo), (gap_hi, _) = epochs
    for name in NAMES:
        assert not np.any(dev[name][..., gap_lo:gap_hi]), (msg, name)
    assert np.all(dev["envelope"][..., gap_lo - 10:gap_lo] > 0), msg
    ref_w = np.stack([orc.cwt_complex(x[ch], FS, f, epoch_bounds=np.array(epochs)) for ch in range(x.shape[0])])
    gate = bm.gate_bound(ref_w, rows, g, h)
    print("%s: largest gate bound: analytic %.3g of max |z| %.3g, power %.3g of max %.3g"
          % (msg, gate[0].max(), np.abs(dev["analytic"]).max(), gate[1].max(), dev["power"].max()))
    _compare(dev, ref_w, rows, g, h, msg, gate=gate)


def test_meets_the_oracle_end_to_end():
    from ghost_amd import engine
    from ghost_amd.synthetic import lfp
    from ghost_amd.wave import ContinuousWaveletTransform, Morse
    n = 5003
    x = lfp(3, n, FS, seed=11)
    epochs = [[0, 2300], [2700, n]]
    freqs = np.geomspace(200.0, 4.0, 14)
    # all 14 rows, as a plan computes them (transform() would drop the rows too slow for the shorter epoch)
    plan = engine.CwtPlan(n, 3, FS, freqs, output="complex", epoch_bounds=epochs)
    result = plan.execute_resident(np.asarray(x, dtype=np.float32))
    g, h = engine.band_weights(freqs, Morse(fs=FS))
    rows = engine.band_rows([(4.0, 40.0), (12.0, 200.0)], freqs)
    assert rows[1, 0] == 0 and rows[0, 0] + rows[0, 1] == 14 and rows[1, 1] > rows[0, 0] > 0            # they overlap
    _meets_the_oracle(_run(result, rows, g, h), x, freqs, rows, g, h, epochs, "plan, 14 rows")
    result.free()
    plan.close()
    # through transform() and bandpass(): freqs= sorts, and the rows below the shorter epoch's lowest frequency are dropped
    # (there the two epochs are a jump in the timestamps: no columns lie between them)
    ts = np.concatenate([np.arange(2300), 2700 + np.arange(n - 2300)]) / FS
    epochs = [[0, 2300], [2300, n]]
    cwt = ContinuousWaveletTransform()
    cwt.transform(x, fs=FS, timestamps=ts, freqs=freqs, multichannel=True, output="complex")
    f = np.array(cwt.frequencies)
    assert 5 <= f.size <= 14 and np.all(np.diff(f) > 0) and f[-1] == 200.0
    bands = [(f[0], 90.0), (50.0, 200.0)]
    got = cwt.bandpass(bands)
    rows = engine.band_rows(bands, f)
    assert rows[0, 0] == 0 and rows[1, 0] + rows[1, 1] == f.size and rows[0, 1] > rows[1, 0] > 0        # they overlap
    np.testing.assert_array_equal(got.rows, rows)
    np.testing.assert_array_equal(got.bands, np.asarray(bands))
    assert len(got.frequencies) == 2 and all(np.array_equal(fb, f[a:a + m]) for fb, (a, m) in zip(got.frequencies, rows))
    np.testing.assert_array_equal(got.time, ts)
    g, h = engine.band_weights(f, cwt.wavelet)
    _meets_the_oracle({name: getattr(got, name) for name in NAMES}, x, f, rows, g, h, epochs, "transform()")


# -- 4. the physical reading -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["morse", "morlet"])
def test_a_tone_reads_its_amplitude(family):
    from ghost_amd.wave import ContinuousWaveletTransform, Morlet
    x = bm.tone()
    cwt = ContinuousWaveletTransform() if family == "morse" else ContinuousWaveletTransform(wavelet=Morlet(w0=6))
    cwt.transform(x, fs=FS, output="complex")                               # the default grid: 10 voices per octave
    got = cwt.bandpass((5.0, 80.0), outputs=("envelope", "power"))
    assert got.analytic is None and got.envelope.shape == got.power.shape == (1, x.size)
    mid = slice(x.size // 2 - 256, x.size // 2 + 256)
    env, pw = got.envelope[0, mid] / 0.7, got.power[0, mid] / 0.49
    print("%s: envelope / A %.4f .. %.4f, power / A^2 %.4f .. %.4f" % (family, env.min(), env.max(), pw.min(), pw.max()))
    assert np.all(np.abs(env - 1) < 0.01) and np.all(np.abs(pw - 1) < 0.01)


# -- 5. with the rest of the surface -----------------------------------------------------------------------------------
def test_composes_with_output_stride_ascending_freqs_and_the_single_channel_call():
    from ghost_amd.engine import band_rows, band_weights
    from ghost_amd.synthetic import lfp
    from ghost_amd.wave import ContinuousWaveletTransform
    n = 6001
    x = lfp(2, n, FS, seed=5)
    ts = 3.25 + np.arange(n) / FS
    kw = dict(timestamps=ts, fs=FS, freq_limits=[16, 250], voices_per_octave=4, multichannel=True, output="complex", dtype=np.float32)
    bands = [(16.0, 40.0), (30.0, 250.0), (60.0, 70.0)]
    full, strided = ContinuousWaveletTransform(), ContinuousWaveletTransform()
    full.transform(x, **kw)
    strided.transform(x, output_stride=4, **kw)
    a, b = full.bandpass(bands), strided.bandpass(bands)
    f = np.array(full.frequencies)
    rows = band_rows(bands, f)
    g, h = band_weights(f, full.wavelet)
    np.testing.assert_array_equal(b.rows, rows)
    np.testing.assert_array_equal(a.time, ts)
    np.testing.assert_array_equal(b.time, ts[::4])
    assert b.analytic.shape == (2, 3, -(-n // 4)) and a.analytic.shape == (2, 3, n)
    # each against the model on its own coefficients, within the rounding bounds ...
    w_full, w_strided = full.fetch(dtype=np.float32), strided.fetch(dtype=np.float32)
    _compare({k: getattr(a, k) for k in NAMES}, w_full, rows, g, h, "full rate")
    _compare({k: getattr(b, k) for k in NAMES}, w_strided, rows, g, h, "stride 4")
    # ... and column j of the strided answer against column 4 j of the full-rate one: what the two sets of rows may differ
    # by (the gate, once for each) plus the rounding of either
    gate = bm.gate_bound(w_full, rows, g, h)
    _compare({k: getattr(b, k) for k in NAMES}, w_full[..., ::4], rows, g, h, "stride 4 against [..., ::4]",
             gate=(2 * gate[0], 2 * gate[1][..., ::4]))

    # the reference's single-channel call: the channel axis is dropped, the band axis stays; ascending freqs=
    one = ContinuousWaveletTransform()
    one.transform(x[1], fs=FS, freqs=[15.0, 20.0, 30.0, 60.0, 80.0, 100.0, 120.0], output="complex", dtype=np.float32)
    got = one.bandpass((20.0, 100.0), outputs=("envelope",))
    assert got.analytic is None and got.power is None
    assert got.envelope.shape == (1, n) and got.envelope.dtype == np.float32
    assert got.rows.tolist() == [[1, 5]] and got.bands.tolist() == [[20.0, 100.0]]
    np.testing.assert_array_equal(got.frequencies[0], [20.0, 30.0, 60.0, 80.0, 100.0])
    np.testing.assert_array_equal(got.time, np.arange(n) / FS)
    w = one.fetch(dtype=np.float32)
    assert w.shape == (7, n)
    g, h = band_weights(one.frequencies, one.wavelet)
    _compare({"envelope": got.envelope[None]}, w[None], [(1, 5)], g, h, "single channel")
    both = one.bandpass([(20.0, 100.0), (15.0, 30.0)], outputs=("power", "analytic"))
    assert both.envelope is None and both.power.shape == (2, n) and both.analytic.shape == (2, n)
    _compare({"analytic": both.analytic[None], "power": both.power[None]}, w[None], [(1, 5), (0, 3)], g, h, "single channel, two bands")


# -- 6. side effects ---------------------------------------------------------------------------------------------------
def test_the_resident_result_is_as_it_was():
    from ghost_amd.synthetic import lfp
    from ghost_amd.wave import ContinuousWaveletTransform
    x = lfp(3, 9000, FS, seed=3)
    kw = dict(fs=FS, freq_limits=[8, 200], voices_per_octave=4, multichannel=True, output="complex")
    events = np.random.default_rng(4).uniform(0.5, 8.5, 25)
    one, twin = ContinuousWaveletTransform(), ContinuousWaveletTransform()
    one.transform(x, **kw)
    twin.transform(x, **kw)
    before = one.triggered(events, before=0.2, after=0.2)
    first = one.bandpass([(8.0, 12.0), (80.0, 200.0)])
    np.testing.assert_array_equal(one.fetch(slice(1, 4), 100, 5000), twin.fetch(slice(1, 4), 100, 5000))
    assert one._pending is not None                                         # still lazy: nothing was brought over
    after = one.triggered(events, before=0.2, after=0.2)
    for name in ("amplitude", "power", "evoked", "vector", "itpc"):
        np.testing.assert_array_equal(getattr(before, name), getattr(after, name), err_msg=name)
    np.testing.assert_array_equal(one.coefficients, twin.coefficients)
    again = one.bandpass([(8.0, 12.0), (80.0, 200.0)])                      # ... and after the result has been brought over
    for name in NAMES:
        np.testing.assert_array_equal(getattr(first, name), getattr(again, name), err_msg=name)
    np.testing.assert_array_equal(one.fetch(), twin.fetch())


def test_error_surface_on_the_device():
    from ghost_amd.synthetic import lfp
    from ghost_amd.wave import ContinuousWaveletTransform
    x = lfp(4, 4096, FS, seed=1)
    kw = dict(fs=FS, freq_limits=[20, 200], voices_per_octave=4)
    cwt = ContinuousWaveletTransform()
    cwt.transform(x, multichannel=True, **kw)                                            # amplitude
    with pytest.raises(ValueError, match="complex"):
        cwt.bandpass((20.0, 60.0))
    cwt = ContinuousWaveletTransform()
    cwt.transform(x, multichannel=True, output="complex", devices=[0, 0], **kw)          # sharded
    with pytest.raises(ValueError, match="devices"):
        cwt.bandpass((20.0, 60.0))
    cwt = ContinuousWaveletTransform()
    cwt.transform(x, multichannel=True, output="complex", **kw)
    with pytest.raises(ValueError, match=r"bands\[1\]"):
        cwt.bandpass([(20.0, 60.0), (1.0, 4.0)])                                          # a band with no rows
    with pytest.raises(ValueError, match="outputs"):
        cwt.bandpass((20.0, 60.0), outputs=())
    assert cwt.bandpass((20.0, 60.0)).power.shape == (4, 1, 4096)                         # ... and it still works
    cwt.release_device()
    with pytest.raises(ValueError, match="transform"):
        cwt.bandpass((20.0, 60.0))
