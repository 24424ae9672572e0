"""ridge() on the MI355X (csrc/ridge.hip, include/ghostcwt.h: gcwt_ridge): row, amplitude and offset against the prescribed
float32 sequences bit for bit and frequency against the float64 model within the derived bound (tests/ridge_model.py), on
random rows; the device library's arctangent against float64; the same bits whatever else is asked for; end to end against
the oracle; the single-channel call; its side effects."""
import ctypes as C
import itertools

import numpy as np
import pytest

import ridge_model as rm
from oracle import ghost_oracle as orc

pytestmark = pytest.mark.gpu

FS = 1000.0
NAMES = ("row", "amplitude", "offset", "frequency")
DTYPES = {"row": np.int32, "amplitude": np.float32, "offset": np.float32, "frequency": np.float32}
S = 23
T, G = 512, 4                                       # GCWT_RIDGE_TILE_COLS, GCWT_RIDGE_GROUP_BANDS
HZ = 250.0

BAND_LISTS = {                                      # those of test_gpu_bandpass.py
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


def _zero_run(n):
    return (n // 3, n // 3 + max(1, n // 5)) if n >= 5 else (0, 0)


def _rows(c, n, seed):
    """(C, S, n) complex64 rows with a run of exactly-zero columns (where there is room); duplicated rows (ties: the lowest
    index must win) in every 7th column, a dominant first row in every 11th and a dominant last row in every 13th; weights e
    in [0.5, 1.5) with e[9] = e[8] for the ties; nu up to 2.5 pi, so the unwrapping integer is not always 0."""
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((c, S, n)) + 1j * rng.standard_normal((c, S, n))).astype(np.complex64)
    w[:, 9, ::7] = w[:, 8, ::7]
    w[:, 8:10, ::21] *= 4                                                   # ... and there the tied pair is the maximum
    w[:, 0, 3::11] *= 8
    w[:, S - 1, 5::13] *= 8
    lo, hi = _zero_run(n)
    w[..., lo:hi] = 0
    e = (0.5 + rng.random(S)).astype(np.float32)
    e[9] = e[8]
    return w, e, (2.5 * np.pi * rng.random(S)).astype(np.float32)


def _segments(n):
    """One table with every boundary the kernel can trip on, as far as n has room: between a lane's two columns (6 | 7) and
    right after it (a one-column segment [7, 8)), inside the zero run (a segment ends there), at the tile edge T - 1 | T and
    at T | T + 1 (one column again, and between the two columns of the next tile's first lane)."""
    cuts = sorted({v for v in (7, 8, _zero_run(n)[0] + 1, T, T + 1) if 0 < v < n})
    edges = [0] + cuts + [n]
    return np.array(list(zip(edges[:-1], edges[1:])), dtype=np.int64)


def _upload(w, pitch):
    """The rows on the device as a resident result; what lies between n_cols and pitch is NaN: read perhaps, never used."""
    from ghost_amd.engine import DeviceBuffer, DeviceResult
    c, s, n = w.shape
    padded = np.full((c, s, pitch), np.nan + 1j * np.nan, np.complex64)
    padded[..., :n] = w
    buf = DeviceBuffer(padded.nbytes)
    buf.upload(padded)
    return DeviceResult(buf, (c, s, n), pitch, True)


def _run(result, bands, e, nu, segments, outputs=NAMES, hz=HZ):
    from ghost_amd import engine
    res = engine.ridge(result, np.asarray(bands, dtype=np.int32), e, nu, hz, segments, outputs)
    try:
        assert (res.n_channels, res.n_bands, res.n_cols, res.outputs) == (result.shape[0], len(bands), result.shape[2], tuple(outputs))
        assert res.nbytes == result.shape[0] * len(bands) * res.pitch * 4 * len(outputs)
        out = res.to_host()
    finally:
        res.free()
    assert tuple(out) == tuple(k for k in NAMES if k in outputs)
    for name in out:
        assert out[name].dtype == DTYPES[name] and out[name].shape == (result.shape[0], len(bands), result.shape[2]), name
    return out


def _same_bits(a, b, msg):
    assert a.dtype == b.dtype and a.shape == b.shape, msg
    a, b = np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)   # (NaN == NaN, -0 != 0)
    assert np.array_equal(a, b), (msg, int(np.count_nonzero(a != b)))


def _check(got, w, bands, e, nu, segments, msg, hz=HZ):
    """row, amplitude, offset bit for bit; frequency within the bound of the float64 model on the device's own row, NaN
    exactly where the definition says.  -> (error / bound, cells whose unwrapping integer was a tie)."""
    want = rm.ranking32(w, bands, e)
    for name in ("row", "amplitude", "offset"):
        assert np.array_equal(got[name], want[name]), (msg, name, int(np.count_nonzero(got[name] != want[name])))
    zero = np.broadcast_to(~np.any(np.asarray(w) != 0, axis=1)[:, None, :], got["row"].shape)    # the columns without signal
    assert np.all(got["row"][zero] == -1) and not np.any(got["amplitude"][zero]) and not np.any(got["offset"][zero])
    assert np.all(np.isnan(got["frequency"][zero])) and np.all(got["row"][~zero] >= 0)
    return rm.frequency_error(got["frequency"], w, got["row"], nu, hz, segments)


# -- 1. the kernel against the models on its own input -------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 3, 9])
def test_kernel_meets_the_models_on_its_own_input(c):
    worst, ties, any_k, atan_worst = 0.0, 0, False, 0.0
    for n, pitch in [(m, _pitch(m)) for m in (1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3)] + [(T + 32, T + 32)]:
        w, e, nu = _rows(c, n, 100 * c + n)
        result = _upload(w, pitch)
        assert result.pitch % 32 == 0
        seg, one = _segments(n), np.array([[0, n]], dtype=np.int64)
        for what, bands in BAND_LISTS.items():
            msg = "C=%d n=%d %s" % (c, n, what)
            got = _run(result, bands, e, nu, seg)
            ratio, loose = _check(got, w, bands, e, nu, seg, msg)
            print("%s: frequency error / bound %.3f (%d ties of the unwrapping)" % (msg, ratio, loose))
            assert ratio <= 1.0, (msg, ratio)
            worst, ties = max(worst, ratio), ties + loose
            f64 = rm.frequency64(w, got["row"], nu, HZ, seg)
            any_k |= bool(np.any(f64["k"][~np.isnan(f64["frequency"])] != 0))
            if what in ("all rows", "G + 1 bands"):                          # ... and with the recording in one piece
                again = _run(result, bands, e, nu, one)
                for name in ("row", "amplitude", "offset"):
                    _same_bits(again[name], got[name], msg + " one segment " + name)
                ratio, loose = _check(again, w, bands, e, nu, one, msg + " one segment")
                assert ratio <= 1.0, (msg, ratio)
                worst, ties = max(worst, ratio), ties + loose
        # the device's arctangent itself: with nu = 0 and hz_per_cycle = float32(2 pi) the sequence leaves frequency = dphi /
        # span exactly (k = 0; scale = 1 or 0.5), so dphi is read back and held to float64 arctan2 of the same float32 (im, re)
        bands = BAND_LISTS["G + 1 bands"]
        raw = _run(result, bands, e, np.zeros(S, np.float32), one, ("row", "frequency"), hz=float(rm.TWO_PI32))
        re, im, span = rm.product32(w, raw["row"], one)
        live = ~np.isnan(raw["frequency"])
        assert np.array_equal(live, (raw["row"] >= 0) & (span > 0)[None, None, :] & ((re != 0) | (im != 0)))
        dphi = (raw["frequency"].astype(np.float64) * span[None, None, :])[live]
        err = np.abs(dphi - np.arctan2(im.astype(np.float64), re.astype(np.float64))[live]).max(initial=0.0)
        print("C=%d n=%d: atan2f against float64 arctan2: worst %.3e rad over %d cells" % (c, n, err, dphi.size))
        atan_worst = max(atan_worst, float(err))
        result.free()
    print("C=%d: worst frequency error / bound %.3f; %d unwrapping ties; worst atan2f error %.3e rad (gate %.3e)"
          % (c, worst, ties, atan_worst, rm.ATAN_GATE))
    assert any_k and atan_worst <= rm.ATAN_GATE


def test_planted_ties_edges_a_flat_parabola_and_large_nu():
    e = np.ones(6, np.float32)
    w = np.zeros((1, 6, 8), np.complex64)
    w[0, :, 0] = [1, 2, 2, 1, 2, 0]                                         # equal maxima: the lowest index wins
    w[0, :, 1] = [3, 1, 1, 1, 1, 1]                                         # the band's first row
    w[0, :, 2] = [1, 1, 1, 1, 1, 3]                                         # ... and its last
    w[0, :, 3] = [0, 1, 3, 2, 0, 0]
    w[0, :, 5] = [1j, 1j, 1j, 1j, 1j, 1j]                                   # all equal: row 0
    w[0, :, 6] = [0, 0, 0, 2, 0, 0]
    w[0, :, 7] = [0, 0, 1, 1, 0, 0]
    result = _upload(w, _pitch(8))
    bands, seg = [(0, 6), (1, 4)], np.array([[0, 8]])
    got = _run(result, bands, e, np.zeros(6, np.float32), seg)
    assert got["row"][0, 0].tolist() == [1, 0, 5, 2, -1, 0, 3, 2] and got["row"][0, 1].tolist() == [1, 1, 1, 2, -1, 1, 3, 2]
    assert got["amplitude"][0, 0].tolist() == [2, 3, 3, 3, 0, 1, 2, 1]
    assert got["offset"][0, 0].tolist() == [0.5, 0, 0, float(np.float32(-1.5) / np.float32(-13)), 0, 0, 0, 0.5]
    assert got["offset"][0, 1].tolist()[:3] == [0, 0, 0]
    _check(got, w, bands, e, np.zeros(6, np.float32), seg, "planted")
    result.free()
    # d2 == 0: qm = 1 - 2^-24, q = qp = 1: qm + qp rounds to 2 and the denominator vanishes
    e2 = np.array([1 - 2.0 ** -24, 1, 1], np.float32)
    w2 = np.ones((1, 3, 2), np.complex64)
    result = _upload(w2, _pitch(2))
    flat = _run(result, [(0, 3)], e2, np.zeros(3, np.float32), np.array([[0, 2]]))
    assert flat["row"].ravel().tolist() == [1, 1] and flat["offset"].view(np.uint32).ravel().tolist() == [0, 0]
    result.free()
    # a row that turns 3.2 times per column: with nu near the true advance the frequency is 3.2 cycles per column
    n = 300
    theta = 2 * np.pi * 3.2
    w3 = np.zeros((1, 3, n), np.complex64)
    w3[0, 1] = (0.7 * np.exp(1j * (theta * np.arange(n) + 0.2))).astype(np.complex64)
    nu = np.array([0.0, theta * 1.02, 0.0], np.float32)
    result = _upload(w3, _pitch(n))
    seg = np.array([[0, 131], [131, n]])
    got = _run(result, [(0, 3)], np.ones(3, np.float32), nu, seg)
    ratio, loose = _check(got, w3, [(0, 3)], np.ones(3, np.float32), nu, seg, "large nu")
    f64 = rm.frequency64(w3, got["row"], nu, HZ, seg)
    assert ratio <= 1.0 and loose == 0 and np.all(f64["k"][0, 0, 1:130] == 6) and np.all(f64["k"][0, 0, [0, 130, 131, n - 1]] == 3)
    assert np.all(np.abs(got["frequency"] / (3.2 * HZ) - 1) < 1e-4)          # (complex64 phases of up to 6000 rad)
    result.free()


def test_rows_and_outputs_that_start_off_16_bytes():
    """The entry point takes any pitch >= n_cols: an odd one moves 8 bytes per column and gives the same bits; nothing is
    stored past n_cols."""
    from ghost_amd import _lib
    from ghost_amd.engine import DeviceBuffer
    c, n = 2, T + 7
    w, e, nu = _rows(c, n, 77)
    bands = np.array(BAND_LISTS["G + 1 bands"], dtype=np.int32)
    seg = _segments(n)
    aligned = _upload(w, _pitch(n))
    want = _run(aligned, bands, e, nu, seg)
    aligned.free()
    odd = _upload(w, n)
    out_pitch = n + 2
    bufs = {}
    for name in NAMES:
        bufs[name] = DeviceBuffer(c * len(bands) * out_pitch * 4)
        bufs[name].upload(np.full((c, len(bands), out_pitch), 7, DTYPES[name]))
    f32p = C.POINTER(C.c_float)
    _lib.check(_lib.lib.gcwt_ridge(odd.buffer.ptr, n, c, S, n, bands.ctypes.data_as(C.POINTER(C.c_int32)), len(bands),
                                   e.ctypes.data_as(f32p), nu.ctypes.data_as(f32p), HZ, seg.ctypes.data_as(C.POINTER(C.c_int64)),
                                   len(seg), bufs["row"].ptr, bufs["amplitude"].ptr, bufs["offset"].ptr, bufs["frequency"].ptr,
                                   out_pitch))
    for name in NAMES:
        got = bufs[name].download((c, len(bands), out_pitch), DTYPES[name])
        _same_bits(np.ascontiguousarray(got[..., :n]), want[name], name)
        assert np.all(got[..., n:] == 7), name
        bufs[name].free()
    odd.free()


# -- 2. the same bits ------------------------------------------------------------------------------------------------------
def test_a_cell_has_the_same_bits_whatever_else_is_asked_for():
    from ghost_amd.engine import DeviceResult
    c, n = 3, 2 * T + 3
    w, e, nu = _rows(c, n, 5)
    result = _upload(w, _pitch(n))
    seg = _segments(n)
    alone = {}
    for what, bands in BAND_LISTS.items():                                  # each band alone against the band inside every list
        got = _run(result, bands, e, nu, seg)
        for at, band in enumerate(bands):
            if band not in alone:
                alone[band] = _run(result, [band], e, nu, seg)
            for name in NAMES:
                _same_bits(np.ascontiguousarray(got[name][:, at:at + 1]), alone[band][name], "%s: %s of band %d" % (what, name, at))
    bands = BAND_LISTS["runs around the depth"]                             # a permuted list
    got = _run(result, bands, e, nu, seg)
    order = np.random.default_rng(1).permutation(len(bands))
    mixed = _run(result, [bands[k] for k in order], e, nu, seg)
    for name in NAMES:
        _same_bits(mixed[name], np.ascontiguousarray(got[name][:, order]), "permuted " + name)
    bands = BAND_LISTS["G + 1 bands"]                                       # every subset of the outputs, and a second run
    full = _run(result, bands, e, nu, seg)
    for k in range(1, len(NAMES) + 1):
        for subset in itertools.combinations(NAMES, k):
            part = _run(result, bands, e, nu, seg, subset)
            for name in subset:
                _same_bits(part[name], full[name], "%s of %s" % (name, "+".join(subset)))
    # the same buffer seen with fewer columns: other tiles are ragged, other lanes take the last column (the last segment ends
    # earlier: only the last column's frequency may change, and it becomes that of a one-sided difference)
    for m in (1, 2, T - 1, T, T + 1, 2 * T, 2 * T + 1, 2 * T + 2):
        view = DeviceResult(result.buffer, (c, S, m), result.pitch, True)
        cut = seg[seg[:, 0] < m].copy()
        cut[-1, 1] = m
        got = _run(view, bands, e, nu, cut)
        for name in ("row", "amplitude", "offset"):
            _same_bits(got[name], np.ascontiguousarray(full[name][..., :m]), "%s first %d columns" % (name, m))
        _same_bits(got["frequency"][..., :m - 1], np.ascontiguousarray(full["frequency"][..., :m - 1]), "frequency first %d columns" % m)
        ratio, _ = _check(got, w[..., :m], bands, e, nu, cut, "first %d columns" % m)
        assert ratio <= 1.0
    result.free()


# -- 3. end to end against the oracle ----------------------------------------------------------------------------------
def _meets_the_oracle(got, ref_w, f, rows, stride, segments, msg):
    """cwt.ridge()'s (C, B, N) arrays against the float64 model on the oracle's coefficients ref_w (C, S, N): row equal outside
    the near-tie columns, at most 1 % of all; amplitude and frequency within what the transform's gate -- eps_r = 1e-5 max_t
    |W_r| on every sample of row r -- allows through the definition, plus the rounding bounds: amplitude moves by eps_row (e =
    1) and 3 roundings; the phase of a neighbour a by asin(eps_row / |a|), so the advance by the two neighbours' sum."""
    e, nu, hz = np.ones(f.size, np.float32), 2 * np.pi * f * stride / FS, FS / stride
    ref = rm.model(ref_w, rows, e, nu, hz, segments)
    tie = rm.near_ties(np.abs(ref_w) ** 2, rows)
    zero = ~np.any(ref_w != 0, axis=1)                                      # C, N: the gap
    tie &= ~zero[:, None, :]
    share = tie.mean()
    assert share <= 0.01, (msg, share)
    assert np.array_equal(got.row[~tie], ref["row"][~tie]), (msg, int(np.count_nonzero(got.row[~tie] != ref["row"][~tie])))
    assert np.all(got.row[np.broadcast_to(zero[:, None, :], got.row.shape)] == -1)
    eps = 1e-5 * np.abs(ref_w).max(axis=-1)                                 # C, S
    ch = np.arange(ref_w.shape[0])[:, None, None]
    eps_row = eps[ch, np.maximum(got.row, 0)]
    bound = eps_row + 3 * rm.U * ref["amplitude"]
    err = np.abs(got.amplitude - ref["amplitude"])
    assert np.all(err[~tie] <= bound[~tie]), (msg, float((err[~tie] / np.maximum(bound[~tie], 1e-300)).max()))
    tm, tp, _ = rm.neighbours(segments, ref_w.shape[-1])
    a, b = np.abs(rm._on_row(ref_w, got.row, tp)), np.abs(rm._on_row(ref_w, got.row, tm))
    with np.errstate(all="ignore"):
        extra = np.arcsin(np.minimum(eps_row / a, 1)) + np.arcsin(np.minimum(eps_row / b, 1))
    extra = np.where(np.isfinite(extra), extra, np.pi)
    ratio, loose = rm.frequency_error(got.frequency, ref_w, got.row, nu, hz, segments, extra_angle=extra)
    print("%s: %.3f %% near ties; amplitude error / bound %.3f; frequency error / bound %.3f (%d unwrapping ties); largest "
          "allowance of the gate %.2e rad" % (msg, 100 * share, float((err[~tie] / np.maximum(bound[~tie], 1e-300)).max()), ratio,
                                              loose, float(extra[got.row >= 0].max())))
    assert ratio <= 1.0, (msg, ratio)
    return ref


@pytest.mark.parametrize("stride", [1, 4])
def test_the_chirp_meets_the_oracle_end_to_end(stride):
    from ghost_amd import engine
    from ghost_amd.wave import ContinuousWaveletTransform
    x = np.stack([rm.chirp(), 0.5 * rm.chirp()[::-1]])
    cwt = ContinuousWaveletTransform()
    cwt.transform(x, fs=FS, freqs=rm.CHIRP_FREQS, multichannel=True, output="complex", output_stride=stride)
    f = np.array(cwt.frequencies)
    assert f.size == rm.CHIRP_FREQS.size and np.all(np.diff(f) > 0)
    bands = [(f[0], f[-1]), (f[0], 80.0), (25.0, f[-1])]                     # (the sweep stays well inside each)
    got = cwt.ridge(bands)
    rows = engine.band_rows(bands, f)
    n = -(-x.shape[1] // stride)
    assert got.row.shape == got.amplitude.shape == got.offset.shape == got.frequency.shape == (2, 3, n)
    np.testing.assert_array_equal(got.rows, rows)
    np.testing.assert_array_equal(got.bands, np.asarray(bands))
    assert len(got.frequencies) == 3 and all(np.array_equal(fb, f[a:a + m]) for fb, (a, m) in zip(got.frequencies, rows))
    ref_w = np.stack([orc.cwt_complex(x[ch], FS, f) for ch in range(2)])[..., ::stride]
    ref = _meets_the_oracle(got, ref_w, f, rows, stride, np.array([[0, n]]), "chirp, stride %d" % stride)
    # the physical reading: the ridge follows the sweep, at either stride
    mid = slice(1500 // stride, n - 1500 // stride)
    inst = (31.0 + (67.0 - 31.0) * np.arange(x.shape[1]) / x.shape[1])[::stride]
    assert np.all(np.abs(got.frequency[0, 0, mid] / inst[mid] - 1) < 0.01)
    assert np.all(np.abs(got.frequency[1, 0, mid] / inst[::-1][mid] - 1) < 0.01)
    assert np.all(np.abs(got.amplitude[0, 0, mid] / 0.8 - 1) < 0.06)
    grid = got.grid_frequency()
    assert grid.shape == got.row.shape and np.all(np.abs(grid[0, 0, mid] / inst[mid] - 1) < 0.03)
    assert np.all(np.abs(got.offset) <= 0.5 + 1e-3) and np.array_equal(ref["row"] < 0, got.row < 0)


@pytest.mark.parametrize("stride", [1, 4])
def test_two_epochs_and_the_single_channel_call(stride):
    from ghost_amd import engine
    from ghost_amd.wave import ContinuousWaveletTransform
    n, cut = 9000, 4001                                                     # the stride divides neither epoch's first sample
    x = rm.chirp(n)
    ts = np.concatenate([np.arange(cut), 700 + np.arange(cut, n)]) / FS
    epochs = np.array([[0, cut], [cut, n]])
    cwt = ContinuousWaveletTransform()
    cwt.transform(x, fs=FS, timestamps=ts, freqs=rm.CHIRP_FREQS, output="complex", output_stride=stride)
    f = np.array(cwt.frequencies)
    assert f.size == rm.CHIRP_FREQS.size
    got = cwt.ridge((f[0], f[-1]))
    cols = -(-n // stride)
    assert got.row.shape == (1, cols) and got.frequency.shape == (1, cols) and got.row.dtype == np.int32    # no channel axis
    np.testing.assert_array_equal(got.time, ts[::stride])
    segments = engine.segments_of(ts[::stride], stride / FS, FS, cols)
    assert segments.tolist() == [[0, -(-cut // stride)], [-(-cut // stride), cols]]
    ref_w = orc.cwt_complex(x, FS, f, epoch_bounds=epochs)[None, :, ::stride]

    class Lifted:                                                           # the channel axis back on
        row, amplitude, frequency, offset = got.row[None], got.amplitude[None], got.frequency[None], got.offset[None]
    _meets_the_oracle(Lifted, ref_w, f, [(0, f.size)], stride, segments, "two epochs, stride %d" % stride)
    # the advance never reaches across the jump: the columns on either side of it are one-sided differences
    edge = int(segments[0, 1])
    one_sided = rm.frequency64(ref_w, Lifted.row, 2 * np.pi * f * stride / FS, FS / stride, segments)["span"]
    assert one_sided[edge - 1] == 1 and one_sided[edge] == 1 and one_sided[edge - 2] == 2
    only = cwt.ridge((f[0], f[-1]), outputs=("frequency",))
    assert only.row is None and only.amplitude is None and only.offset is None
    assert np.array_equal(only.frequency.view(np.uint32), got.frequency.view(np.uint32))
    with pytest.raises(ValueError, match="row.*offset"):
        only.grid_frequency()


# -- 4. side effects -----------------------------------------------------------------------------------------------------
def test_the_resident_result_is_as_it_was():
    from ghost_amd.synthetic import lfp
    from ghost_amd.wave import ContinuousWaveletTransform
    x = lfp(3, 9000, FS, seed=3)
    kw = dict(fs=FS, freq_limits=[8, 200], voices_per_octave=4, multichannel=True, output="complex")
    one, twin = ContinuousWaveletTransform(), ContinuousWaveletTransform()
    one.transform(x, **kw)
    twin.transform(x, **kw)
    before = one.bandpass([(8.0, 12.0), (80.0, 200.0)])
    first = one.ridge([(8.0, 12.0), (80.0, 200.0)])
    np.testing.assert_array_equal(one.fetch(slice(1, 4), 100, 5000), twin.fetch(slice(1, 4), 100, 5000))
    assert one._pending is not None                                         # still lazy: nothing was brought over
    after = one.bandpass([(8.0, 12.0), (80.0, 200.0)])
    for name in ("analytic", "envelope", "power"):
        np.testing.assert_array_equal(getattr(before, name), getattr(after, name), err_msg=name)
    np.testing.assert_array_equal(one.coefficients, twin.coefficients)
    again = one.ridge([(8.0, 12.0), (80.0, 200.0)])                         # ... and after the result has been brought over
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
        cwt.ridge((20.0, 60.0))
    cwt = ContinuousWaveletTransform()
    cwt.transform(x, multichannel=True, output="complex", devices=[0, 0], **kw)          # sharded
    with pytest.raises(ValueError, match="devices"):
        cwt.ridge((20.0, 60.0))
    cwt = ContinuousWaveletTransform()
    cwt.transform(x, multichannel=True, output="complex", **kw)
    with pytest.raises(ValueError, match=r"bands\[1\]"):
        cwt.ridge([(20.0, 60.0), (1.0, 4.0)])                                             # a band with no rows
    with pytest.raises(ValueError, match="outputs"):
        cwt.ridge((20.0, 60.0), outputs=())
    assert cwt.ridge((20.0, 60.0)).row.shape == (4, 1, 4096)                              # ... and it still works
    cwt.release_device()
    with pytest.raises(ValueError, match="transform"):
        cwt.ridge((20.0, 60.0))
