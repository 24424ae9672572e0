"""squeeze() on the MI355X (csrc/squeeze.hip, include/ghostcwt.h: gcwt_squeeze): frequency against the float64 model within
ridge's derived bound, index and the sums against the prescribed float32 steps bit for bit on the device's own frequency and
index (tests/squeeze_model.py), on random rows; planted edges; the same bits whatever else is asked for; the ties to ridge()
and bandpass(); end to end against the oracle; epochs, the single-channel call and the side effects."""
import ctypes as C
import itertools

import numpy as np
import pytest

import ridge_model as rm
import squeeze_model as sm
from bandpass_model import norm2_32

pytestmark = pytest.mark.gpu

FS = 1000.0
NAMES = ("coefficients", "power", "frequency", "index")
DTYPES = {"coefficients": np.complex64, "power": np.float32, "frequency": np.float32, "index": np.int32}
S = 23
T, G = 512, 16                                      # GCWT_SQUEEZE_TILE_COLS, GCWT_SQUEEZE_GROUP_CELLS
HZ = 250.0
RUNS = ((0, S), (7, 1), (3, 17))


def _pitch(n):
    from ghost_amd.engine import _pitch
    return _pitch(n)


def _zero_run(n):
    return (n // 3, n // 3 + max(1, n // 5)) if n >= 5 else (0, 0)


def _rows(c, n, seed):
    """(C, S, n) complex64 rows with a run of exactly-zero columns (where there is room), as test_gpu_ridge.py makes them;
    weights g of either sign; floor2 in [0.4, 1.2): |w|^2 is exponential with mean 2, so about a third of the entries is out;
    nu up to 2.5 pi, so the unwrapping integer is not always 0."""
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((c, S, n)) + 1j * rng.standard_normal((c, S, n))).astype(np.complex64)
    w[:, 0, 3::11] *= 8
    w[:, S - 1, 5::13] *= 8
    lo, hi = _zero_run(n)
    w[..., lo:hi] = 0
    g = rng.standard_normal(S).astype(np.float32)
    floor2 = (0.4 + 0.8 * rng.random(S)).astype(np.float32)
    return w, g, floor2, (2.5 * np.pi * rng.random(S)).astype(np.float32)


def _segments(n):
    """test_gpu_ridge.py's table: boundaries between a lane's two columns (6 | 7) and right after it (a one-column segment
    [7, 8)), inside the zero run, at the tile edge T - 1 | T and at T | T + 1, as far as n has room."""
    cuts = sorted({v for v in (7, 8, _zero_run(n)[0] + 1, T, T + 1) if 0 < v < n})
    edges = [0] + cuts + [n]
    return np.array(list(zip(edges[:-1], edges[1:])), dtype=np.int64)


def _edges(n_cells):
    """With hz = 250 and nu up to 2.5 pi the frequencies spread over about -125 .. 440 Hz: these cells leave some below
    edges[0] and some at or above edges[L]."""
    return np.geomspace(8.0, 260.0, n_cells + 1).astype(np.float32)


def _upload(w, pitch):
    """The rows on the device as a resident result; what lies between n_cols and pitch is NaN: read perhaps, never used."""
    from ghost_amd.engine import DeviceBuffer, DeviceResult
    c, s, n = w.shape
    padded = np.full((c, s, pitch), np.nan + 1j * np.nan, np.complex64)
    padded[..., :n] = w
    buf = DeviceBuffer(padded.nbytes)
    buf.upload(padded)
    return DeviceResult(buf, (c, s, n), pitch, True)


def _run(result, rows, g, floor2, nu, segments, edges, descending, outputs=NAMES, hz=HZ):
    from ghost_amd import engine
    res = engine.squeeze(result, rows, g, floor2, nu, hz, segments, edges, descending, outputs)
    c, n, n_cells = result.shape[0], result.shape[2], len(edges) - 1
    lead = {"coefficients": n_cells, "power": n_cells, "frequency": rows[1], "index": rows[1]}
    try:
        assert (res.n_channels, res.n_rows, res.n_cells, res.n_cols, res.outputs) == (c, rows[1], n_cells, n, tuple(outputs))
        assert res.nbytes == sum(c * lead[k] * res.pitch * np.dtype(DTYPES[k]).itemsize for k in outputs)
        out = res.to_host()
    finally:
        res.free()
    assert tuple(out) == tuple(k for k in NAMES if k in outputs)
    for name in out:
        assert out[name].dtype == DTYPES[name] and out[name].shape == (c, lead[name], n), name
    return out


def _same_bits(a, b, msg):
    assert a.dtype == b.dtype and a.shape == b.shape, msg
    a, b = np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)   # (NaN == NaN, -0 != 0)
    assert np.array_equal(a, b), (msg, int(np.count_nonzero(a != b)))


def _check(got, w, rows, g, floor2, nu, segments, edges, descending, msg, hz=HZ):
    """(a) frequency within the bound of the float64 model, NaN exactly where the definition says; (b) index bit for bit the
    definition's on the device's own frequency; (c) coefficients and power bit for bit the float32 chain over the device's own
    index; (d) the float64 model's index differs only where it cannot decide.  -> (frequency error / bound, unwrapping ties,
    entries where the two indices differ)."""
    c, _, n = w.shape
    ratio, loose = rm.frequency_error(got["frequency"], w, sm.every_row(rows[0], rows[1], c, n), nu, hz, segments)
    assert ratio <= 1.0, (msg, ratio)
    want = sm.index32(got["frequency"], w, rows, floor2, edges, descending)
    assert np.array_equal(got["index"], want), (msg, int(np.count_nonzero(got["index"] != want)))
    chain = sm.chain32(w, rows, g, got["index"], len(edges) - 1)
    _same_bits(got["coefficients"], chain["coefficients"], msg + " coefficients")
    _same_bits(got["power"], chain["power"], msg + " power")
    ref = sm.model(w, rows, g, floor2, nu, hz, segments, edges, descending)
    differ = got["index"] != ref["index"]
    assert not np.any(differ & ~ref["undecidable"]), (msg, int(np.count_nonzero(differ & ~ref["undecidable"])))
    zero = ~np.any(np.asarray(w) != 0, axis=1)                              # the columns without signal
    assert np.all(got["index"][np.broadcast_to(zero[:, None, :], got["index"].shape)] == -1)
    wide = np.broadcast_to(zero[:, None, :], got["power"].shape)
    assert not np.any(got["coefficients"].view(np.uint32).reshape(got["power"].shape + (2,))[wide]) and not np.any(got["power"][wide])
    return ratio, loose, int(np.count_nonzero(differ))


# -- 1. the kernel against the models on its own input -------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 3])
def test_kernel_meets_the_models_on_its_own_input(c):
    worst, ties, moved, atan_worst, out_share, below, above = 0.0, 0, 0, 0.0, [], False, False
    cells = (1, 2, G - 1, G, G + 1, 2 * G + 1)
    for n in (1, 2, 7, T - 1, T, T + 1, 2 * T + 3):
        w, g, floor2, nu = _rows(c, n, 100 * c + n)
        result = _upload(w, _pitch(n))
        seg, one = _segments(n), np.array([[0, n]], dtype=np.int64)
        for n_cells in cells:
            edges = _edges(n_cells)
            for rows, descending in itertools.product(RUNS, (False, True)):
                msg = "C=%d n=%d L=%d rows=%r descending=%d" % (c, n, n_cells, rows, descending)
                got = _run(result, rows, g, floor2, nu, seg, edges, descending)
                ratio, loose, differ = _check(got, w, rows, g, floor2, nu, seg, edges, descending, msg)
                worst, ties, moved = max(worst, ratio), ties + loose, moved + differ
                f = got["frequency"]
                with np.errstate(invalid="ignore"):
                    below, above = below or bool(np.any(f < edges[0])), above or bool(np.any(f >= edges[-1]))
                if n >= T:
                    out_share.append(float((~sm.inside32(w, rows, floor2))[..., :_zero_run(n)[0]].mean()))   # of the live columns
        # with the recording in one piece, the other direction, all rows
        got = _run(result, RUNS[0], g, floor2, nu, one, _edges(G + 1), True)
        _check(got, w, RUNS[0], g, floor2, nu, one, _edges(G + 1), True, "C=%d n=%d one segment" % (c, n))
        # the device's arctangent itself: with nu = 0 and hz_per_cycle = float32(2 pi) the sequence leaves frequency = dphi /
        # span exactly (k = 0; scale = 1 or 0.5), so dphi is read back and held to float64 arctan2 of the same float32 (im, re)
        raw = _run(result, RUNS[0], g, floor2, np.zeros(S, np.float32), one, _edges(1), False, ("frequency",), hz=float(rm.TWO_PI32))
        re, im, span = rm.product32(w, sm.every_row(0, S, c, n), one)
        live = ~np.isnan(raw["frequency"])
        assert np.array_equal(live, (span > 0)[None, None, :] & ((re != 0) | (im != 0)))
        dphi = (raw["frequency"].astype(np.float64) * span[None, None, :])[live]
        err = np.abs(dphi - np.arctan2(im.astype(np.float64), re.astype(np.float64))[live]).max(initial=0.0)
        print("C=%d n=%d: atan2f against float64 arctan2: worst %.3e rad over %d entries" % (c, n, err, dphi.size))
        atan_worst = max(atan_worst, float(err))
        result.free()
    print("C=%d: worst frequency error / bound %.3f; %d unwrapping ties; %d entries where the float64 model names another cell "
          "(all undecidable); %.3f of the entries below the threshold; worst atan2f error %.3e rad (gate %.3e)"
          % (c, worst, ties, moved, float(np.mean(out_share)), atan_worst, rm.ATAN_GATE))
    assert below and above and 0.25 <= np.mean(out_share) <= 0.42 and atan_worst <= rm.ATAN_GATE


# -- 2. planted edges ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("descending", [False, True])
def test_an_entry_on_an_edge_goes_to_the_cell_above_and_one_on_the_last_edge_is_out(descending):
    c, n = 2, T + 9
    w, g, _, nu = _rows(c, n, 31)
    floor2 = np.zeros(S, np.float32)
    result = _upload(w, _pitch(n))
    seg = _segments(n)
    first = _run(result, (0, S), g, floor2, nu, seg, _edges(3), descending, ("frequency",))["frequency"]
    pool = np.unique(first[np.isfinite(first) & (first > 1.0)])
    edges = pool[np.linspace(0, pool.size - 1, 2 * G + 2).astype(int)]       # 2G + 1 cells, every edge a frequency of an entry
    assert edges.dtype == np.float32 and np.all(np.diff(edges) > 0)
    got = _run(result, (0, S), g, floor2, nu, seg, edges, descending)
    _same_bits(got["frequency"], first, "frequency")
    live = norm2_32(w) > 0
    n_cells = edges.size - 1
    for l, edge in enumerate(edges):
        on = (got["frequency"] == edge) & live
        assert np.any(on), l
        if l == n_cells:
            assert np.all(got["index"][on] == -1)
        else:
            assert np.all(got["index"][on] == (n_cells - 1 - l if descending else l)), l
    _check(got, w, (0, S), g, floor2, nu, seg, edges, descending, "planted edges")
    result.free()


# -- 3. the same bits ----------------------------------------------------------------------------------------------------
def test_an_entry_has_the_same_bits_whatever_else_is_asked_for():
    from ghost_amd.engine import DeviceResult
    c, n, rows, n_cells = 3, 2 * T + 3, (3, 17), 2 * G + 1
    w, g, floor2, nu = _rows(c, n, 5)
    result = _upload(w, _pitch(n))
    seg, edges = _segments(n), _edges(n_cells)
    full = _run(result, rows, g, floor2, nu, seg, edges, True)
    _check(full, w, rows, g, floor2, nu, seg, edges, True, "full")
    for k in range(1, len(NAMES) + 1):                                      # every subset of the outputs (and so a second run)
        for subset in itertools.combinations(NAMES, k):
            part = _run(result, rows, g, floor2, nu, seg, edges, True, subset)
            for name in subset:
                _same_bits(part[name], full[name], "%s of %s" % (name, "+".join(subset)))
    # the same cells asked for in two calls: what falls outside a call's cells is out there, everything else is as it was
    for descending in (False, True):
        whole = full if descending else _run(result, rows, g, floor2, nu, seg, edges, False)
        lo = _run(result, rows, g, floor2, nu, seg, edges[:G + 2], descending)         # cells 0 .. G
        hi = _run(result, rows, g, floor2, nu, seg, edges[G + 1:], descending)         # cells G + 1 .. 2G
        parts = (hi, lo) if descending else (lo, hi)                                    # in output-row order
        for name in ("coefficients", "power"):
            _same_bits(np.concatenate([parts[0][name], parts[1][name]], axis=1), whole[name], "two calls: " + name)
        shift = parts[0]["power"].shape[1]
        joined = np.where(parts[0]["index"] >= 0, parts[0]["index"], np.where(parts[1]["index"] >= 0, parts[1]["index"] + shift, -1))
        assert np.array_equal(joined, whole["index"]) and not np.any((parts[0]["index"] >= 0) & (parts[1]["index"] >= 0))
        _same_bits(lo["frequency"], whole["frequency"], "two calls: frequency")
    # the same buffer seen with fewer columns: other tiles are ragged, other lanes take the last column (the last segment ends
    # earlier: only the last column's entries may change -- its frequency becomes that of a one-sided difference)
    for m in (1, 2, T - 1, T, T + 1, 2 * T, 2 * T + 1):
        view = DeviceResult(result.buffer, (c, S, m), result.pitch, True)
        cut = seg[seg[:, 0] < m].copy()
        cut[-1, 1] = m
        got = _run(view, rows, g, floor2, nu, cut, edges, True)
        for name in NAMES:
            _same_bits(got[name][..., :m - 1], np.ascontiguousarray(full[name][..., :m - 1]), "%s first %d columns" % (name, m))
        _check(got, w[..., :m], rows, g, floor2, nu, cut, edges, True, "first %d columns" % m)
    result.free()


def test_rows_and_outputs_that_start_off_16_bytes_and_odd_pitches():
    """The entry point takes any pitch >= n_cols and any 8-byte (4-byte) aligned plane: those move 8 bytes per column and
    give the same bits; nothing is stored past n_cols."""
    from ghost_amd import _lib
    from ghost_amd.engine import DeviceBuffer
    c, n, rows, n_cells = 2, T + 7, (0, S), G + 1
    w, g, floor2, nu = _rows(c, n, 77)
    seg, edges = _segments(n), _edges(n_cells)
    aligned = _upload(w, _pitch(n))
    want = _run(aligned, rows, g, floor2, nu, seg, edges, True)
    aligned.free()
    f32p = C.POINTER(C.c_float)
    lead = {"coefficients": n_cells, "power": n_cells, "frequency": S, "index": S}
    # (input pitch, output pitch, bytes that the input and every plane start off 16)
    for pitch, out_pitch, off in ((n, n + 2, 0), (n + 1, n, 0), (n + 1, n + 1, 8), (n + 2, n + 4, 8)):
        padded = np.full((c, S, pitch), np.nan + 1j * np.nan, np.complex64)
        padded[..., :n] = w
        src = DeviceBuffer(padded.nbytes + 16)
        src.upload(padded, off)
        bufs = {}
        for name in NAMES:
            bufs[name] = DeviceBuffer(c * lead[name] * out_pitch * np.dtype(DTYPES[name]).itemsize + 16)
            bufs[name].upload(np.full((c, lead[name], out_pitch), 7, DTYPES[name]), off)
        ptr = {name: C.c_void_p(bufs[name].ptr.value + off) for name in NAMES}
        _lib.check(_lib.lib.gcwt_squeeze(C.c_void_p(src.ptr.value + off), pitch, c, S, n, rows[0], rows[1], g.ctypes.data_as(f32p),
                                         floor2.ctypes.data_as(f32p), nu.ctypes.data_as(f32p), HZ,
                                         seg.ctypes.data_as(C.POINTER(C.c_int64)), len(seg), edges.ctypes.data_as(f32p), n_cells, 1,
                                         ptr["coefficients"], ptr["power"], ptr["frequency"], ptr["index"], out_pitch))
        for name in NAMES:
            got = bufs[name].download((c, lead[name], out_pitch), DTYPES[name], off)
            _same_bits(np.ascontiguousarray(got[..., :n]), want[name], "%s at pitch %d / %d, off %d" % (name, pitch, out_pitch, off))
            assert np.all(got[..., n:] == 7), name
            bufs[name].free()
        src.free()


# -- 4. ties to the neighbours ---------------------------------------------------------------------------------------------
def test_frequency_is_ridges_and_one_cell_is_bandpass():
    from ghost_amd import engine
    c, n = 3, 2 * T + 3
    w, g, floor2, nu = _rows(c, n, 9)
    result = _upload(w, _pitch(n))
    seg = _segments(n)
    e = (0.5 + np.random.default_rng(2).random(S)).astype(np.float32)
    bands = np.array([(0, S), (3, 17), (7, 1)], dtype=np.int32)
    res = engine.ridge(result, bands, e, nu, HZ, seg, ("row", "frequency"))
    ridge = res.to_host()
    res.free()
    got = _run(result, (0, S), g, floor2, nu, seg, _edges(G), False, ("frequency",))["frequency"]
    for b in range(len(bands)):
        row = ridge["row"][:, b]
        on = np.take_along_axis(got, np.maximum(row, 0)[:, None, :], axis=1)[:, 0]
        won = row >= 0
        assert np.any(won) and np.all(np.isnan(ridge["frequency"][:, b][~won]))
        _same_bits(on[won], ridge["frequency"][:, b][won], "ridge band %d" % b)
    # one cell over everything and no threshold: bandpass's analytic wherever no entry of the column is out
    zero = np.zeros(S, np.float32)
    wide = np.array([1e-30, 1e30], np.float32)
    for rows in RUNS:
        one = _run(result, rows, g, zero, nu, seg, wide, False, ("coefficients", "index"))
        res = engine.bandpass(result, np.array([rows], dtype=np.int32), g, None, ("analytic",))
        band = res.to_host()["analytic"]
        res.free()
        whole = np.all(one["index"] == 0, axis=1)                           # C, n
        assert set(np.unique(one["index"]).tolist()) == {-1, 0} and 0 < whole.mean() < 1
        _same_bits(one["coefficients"][:, 0][whole], band[:, 0][whole], "one cell, rows %r" % (rows,))
    result.free()


# -- 5. end to end against the oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["morse", "morlet"])
@pytest.mark.parametrize("stride", [1, 4])
def test_the_chirp_meets_the_oracle_end_to_end(kind, stride):
    """Figures measured on an MI355X are in profiles/squeeze.md."""
    from ghost_amd import engine
    from ghost_amd.wave import ContinuousWaveletTransform, Morlet
    case = sm.chirp_case(kind, stride)
    x, f, m = case["x"], case["f"], case["model"]
    cwt = ContinuousWaveletTransform(wavelet=Morlet(w0=6)) if kind == "morlet" else ContinuousWaveletTransform()
    cwt.transform(x, fs=FS, freqs=f, multichannel=True, output="complex", output_stride=stride)
    assert np.array_equal(np.array(cwt.frequencies), f)
    got = cwt.squeeze(sm.BINS, min_amplitude=sm.MIN_AMPLITUDE, outputs=NAMES)
    n, rows = case["n"], (0, f.size)
    assert got.coefficients.shape == got.power.shape == (2, sm.BINS, n) and got.frequency.shape == got.index.shape == (2, f.size, n)
    assert [getattr(got, k).dtype for k in NAMES] == [DTYPES[k] for k in NAMES]
    assert np.array_equal(got.bin_frequencies, case["centres"]) and np.array_equal(got.edges, case["edges"]) and got.rows == rows
    assert np.array_equal(got.frequencies, f) and got.min_amplitude == sm.MIN_AMPLITUDE
    assert got.time.shape == (n,) and np.allclose(np.diff(got.time), stride / FS)
    # frequency on the entries above the threshold, within what the gate allows on top of the rounding
    above, decidable = m["above"], m["decidable"]
    ratio, loose = sm.frequency_error(got.frequency, case["ref_w"], rows, m["nu"], m["hz"], case["segments"], above, m["extra"])
    # index on every entry the model can decide
    wrong = (got.index != m["index"]) & decidable
    share = float((above & ~decidable).sum() / above.sum())
    print("%s, stride %d: frequency error / bound %.3f (%d unwrapping ties); %.2f %% of the %d entries above the threshold "
          "undecidable; %d decidable entries with another index; %d of all entries differ"
          % (kind, stride, ratio, loose, 100 * share, above.sum(), wrong.sum(), (got.index != m["index"]).sum()))
    assert ratio <= 1.0 and share <= sm.UNDECIDABLE_CAP
    assert not np.any(wrong), int(wrong.sum())
    # the physical reading: sharper than the rows, and as sharp as the model says
    mid = slice(1500 // stride, n - 1500 // stride)
    for ch, inst in enumerate((sm.chirp_frequency(x.shape[1], stride), sm.chirp_frequency(x.shape[1], stride)[::-1])):
        dev = sm.concentration(got.power[ch], case["centres"], inst, mid)
        ref = sm.concentration(m["power"][ch], case["centres"], inst, mid)
        rows_share = sm.concentration(case["h"][:, None] * np.abs(case["ref_w"][ch]) ** 2, f, inst, mid)
        print("channel %d: power in the true cell +-1: %.4f (model %.4f); h |W|^2 in the true row +-1: %.4f" % (ch, dev, ref, rows_share))
        assert dev >= ref - 0.01 and dev > rows_share
    # still invertible: the cells of a column add up to the kept entries' weighted sum, on the device's own rows
    w_dev = cwt.fetch(dtype=np.float32).astype(np.complex128)
    g = case["g"].astype(np.float64)
    kept = got.index >= 0
    want = np.einsum("r,crt->ct", g, np.where(kept, w_dev, 0))
    total = np.einsum("r,crt->ct", np.abs(g), np.abs(w_dev))
    clean = ~np.any(above & ~decidable, axis=1)                             # columns without an undecidable entry
    err = np.abs(got.coefficients.astype(np.complex128).sum(axis=1) - want)
    assert np.all(err[clean] <= f.size * 2.0 ** -23 * total[clean]), float((err[clean] / total[clean]).max())
    real = (got.coefficients.real.sum(axis=1)[0] - x[0, ::stride])[mid]
    print("sum over the cells against the signal, mid-recording: worst %.3f of amplitude 0.8" % np.abs(real).max())
    assert engine.squeeze_edges(case["centres"])[1] is False


# -- 6. epochs, the single-channel call, side effects ------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [1, 4])
def test_two_epochs_and_the_single_channel_call(stride):
    from ghost_amd import engine
    from ghost_amd.wave import ContinuousWaveletTransform
    from ghost_amd.wave.morse import Morse
    from oracle import ghost_oracle as orc
    n, cut = 9000, 4001                                                     # the stride divides neither epoch's first sample
    x = rm.chirp(n)
    ts = np.concatenate([np.arange(cut), 700 + np.arange(cut, n)]) / FS
    epochs = np.array([[0, cut], [cut, n]])
    cwt = ContinuousWaveletTransform()
    cwt.transform(x, fs=FS, timestamps=ts, freqs=rm.CHIRP_FREQS, output="complex", output_stride=stride)
    f = np.array(cwt.frequencies)
    got = cwt.squeeze(min_amplitude=sm.MIN_AMPLITUDE, outputs=NAMES)         # bins=None: the rows' own frequencies
    cols = -(-n // stride)
    assert got.coefficients.shape == got.power.shape == got.frequency.shape == got.index.shape == (f.size, cols)   # no channel axis
    assert np.array_equal(got.bin_frequencies, f) and got.edges.shape == (f.size + 1,) and got.index.dtype == np.int32
    np.testing.assert_array_equal(got.time, ts[::stride])
    segments = engine.segments_of(ts[::stride], stride / FS, FS, cols)
    assert segments.tolist() == [[0, -(-cut // stride)], [-(-cut // stride), cols]]
    ref_w = orc.cwt_complex(x, FS, f, epoch_bounds=epochs)[None, :, ::stride]
    wavelet = Morse(fs=FS, gamma=3.0, beta=20.0)
    g, e = engine.band_weights(f, wavelet)[0], engine.ridge_weights(f, wavelet)
    edges, descending = engine.squeeze_edges(f)
    assert np.array_equal(got.edges, edges) and not descending
    m = sm.oracle_case(ref_w, f, (0, f.size), e, g, stride, FS, segments, edges, descending)
    ratio, loose = sm.frequency_error(got.frequency[None], ref_w, (0, f.size), m["nu"], m["hz"], segments, m["above"], m["extra"])
    wrong = (got.index[None] != m["index"]) & m["decidable"]
    share = float((m["above"] & ~m["decidable"]).sum() / m["above"].sum())
    print("two epochs, stride %d: frequency error / bound %.3f; %.2f %% undecidable; %d decidable entries with another index"
          % (stride, ratio, 100 * share, wrong.sum()))
    assert ratio <= 1.0 and not np.any(wrong)
    # the advance never reaches across the jump: the columns on either side of it are one-sided differences, and a table that
    # joins the two epochs gives other frequencies there and nowhere else
    edge = int(segments[0, 1])
    span = rm.neighbours(segments, cols)[2]
    assert span[edge - 1] == 1 and span[edge] == 1 and span[edge - 2] == 2
    result = cwt.device_result
    joined = engine.squeeze(result, (0, f.size), g, m["floor2"], m["nu"], m["hz"], np.array([[0, cols]]), edges, descending, ("frequency",))
    other = joined.to_host()["frequency"][0]
    joined.free()
    changed = np.flatnonzero(np.any(other.view(np.uint32) != got.frequency.view(np.uint32), axis=0))
    assert changed.tolist() == [edge - 1, edge]
    # columns without signal (a gap between epochs): exact zeros, -1, no frequency
    padded = np.zeros((1, f.size, 64), np.complex64)
    padded[..., :20] = cwt.fetch(dtype=np.float32)[:, 100:120]
    padded[..., 40:] = cwt.fetch(dtype=np.float32)[:, 200:224]
    gap = _upload(padded, _pitch(64))
    out = _run(gap, (0, f.size), g, m["floor2"], m["nu"].astype(np.float32), np.array([[0, 20], [20, 40], [40, 64]]), edges, False, hz=m["hz"])
    assert np.all(out["index"][..., 20:40] == -1) and np.all(np.isnan(out["frequency"][..., 20:40]))
    assert not np.any(out["coefficients"][..., 20:40].view(np.uint32)) and not np.any(out["power"][..., 20:40].view(np.uint32))
    assert np.any(out["index"][..., :20] >= 0) and np.any(out["index"][..., 40:] >= 0)
    gap.free()
    only = cwt.squeeze(min_amplitude=sm.MIN_AMPLITUDE, outputs=("power",))
    assert only.coefficients is None and only.frequency is None and only.index is None
    assert np.array_equal(only.power.view(np.uint32), got.power.view(np.uint32))


def test_the_resident_result_is_as_it_was():
    from ghost_amd.synthetic import lfp
    from ghost_amd.wave import ContinuousWaveletTransform
    x = lfp(3, 9000, FS, seed=3)
    kw = dict(fs=FS, freq_limits=[8, 200], voices_per_octave=4, multichannel=True, output="complex")
    one, twin = ContinuousWaveletTransform(), ContinuousWaveletTransform()
    one.transform(x, **kw)
    twin.transform(x, **kw)
    before = one.bandpass([(8.0, 12.0), (80.0, 200.0)])
    first = one.squeeze(24, freq_limits=(8.0, 100.0), min_amplitude=0.01, outputs=NAMES)       # the default grid descends
    rows = first.rows
    assert first.coefficients.shape == (3, 24, 9000) and first.index.shape == (3, rows[1], 9000) and rows[1] < len(one.frequencies)
    assert np.all(np.diff(first.bin_frequencies) < 0) and np.all(np.diff(first.edges) > 0) and first.index.max() == 23
    # ... and there output row k is the cell of bin_frequencies[k]: the entries of a row lie between that cell's edges
    k = 5
    fk = first.frequency[first.index == k]
    assert fk.size and np.all(fk >= first.edges[23 - k]) and np.all(fk < first.edges[24 - k])
    np.testing.assert_array_equal(one.fetch(slice(1, 4), 100, 5000), twin.fetch(slice(1, 4), 100, 5000))
    assert one._pending is not None                                         # still lazy: nothing was brought over
    after = one.bandpass([(8.0, 12.0), (80.0, 200.0)])
    for name in ("analytic", "envelope", "power"):
        np.testing.assert_array_equal(getattr(before, name), getattr(after, name), err_msg=name)
    np.testing.assert_array_equal(one.coefficients, twin.coefficients)
    again = one.squeeze(24, freq_limits=(8.0, 100.0), min_amplitude=0.01, outputs=NAMES)       # ... and after the result came over
    for name in NAMES:
        _same_bits(getattr(first, name), getattr(again, name), name)
    np.testing.assert_array_equal(one.fetch(), twin.fetch())
    np.testing.assert_array_equal(one.frequencies, twin.frequencies)


def test_error_surface_on_the_device():
    from ghost_amd.synthetic import lfp
    from ghost_amd.wave import ContinuousWaveletTransform
    x = lfp(4, 4096, FS, seed=1)
    kw = dict(fs=FS, freq_limits=[20, 200], voices_per_octave=4)
    cwt = ContinuousWaveletTransform()
    cwt.transform(x, multichannel=True, **kw)                                            # amplitude
    with pytest.raises(ValueError, match="complex"):
        cwt.squeeze()
    cwt = ContinuousWaveletTransform()
    cwt.transform(x, multichannel=True, output="complex", devices=[0, 0], **kw)          # sharded
    with pytest.raises(ValueError, match="devices"):
        cwt.squeeze()
    cwt = ContinuousWaveletTransform()
    cwt.transform(x, multichannel=True, output="complex", **kw)
    with pytest.raises(ValueError, match="freq_limits"):
        cwt.squeeze(freq_limits=(1.0, 4.0))                                               # no rows
    with pytest.raises(ValueError, match="outputs"):
        cwt.squeeze(outputs=())
    with pytest.raises(ValueError, match="'bins'"):
        cwt.squeeze(1)
    got = cwt.squeeze()                                                                   # ... and it still works
    assert got.coefficients.shape == (4, len(cwt.frequencies), 4096) and got.power is None
    cwt.release_device()
    with pytest.raises(ValueError, match="transform"):
        cwt.squeeze()
