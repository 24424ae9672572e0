"""NumPy twins of gcwt_ridge's definition (include/ghostcwt.h): the spectral ridge of a band and the frequency on it.

W (C, S, n_cols) complex; a band is the rows first .. first + R - 1; e (S,) > 0; nu (S,) >= 0; segments (n, 2) of (start,
stop), covering [0, n_cols).  For a channel c, a band and a column t, with q_r = e_r |W[c, r, t]|^2:
    row = the lowest r among the largest q_r, -1 where all are 0;   amplitude = sqrt(q_row);
    offset = 0.5 (qm - qp) / (qm + qp - 2 q_row), qm and qp the q of rows row -+ 1; 0 on the band's first and last row, where
        the denominator is 0, and with no winner;
    frequency = (dphi + 2 pi k) / (2 pi span) hz_per_cycle,  dphi = arg(W[c, row, tp] conj(W[c, row, tm])),  tm = max(t - 1,
        start), tp = min(t + 1, stop - 1), span = tp - tm,  k = rint((span nu_row - dphi) / (2 pi)); NaN where row == -1,
        span == 0, or the product is 0.

Two models.  ``model`` is the definition in float64.  ``ranking32`` and ``product32`` are the prescribed float32 sequences
themselves (csrc/ridge.hip), bit for bit: row, amplitude, offset, and the (re, im) that the arctangent is taken of.  The
arctangent is the device library's and is not modelled: ``frequency64`` evaluates the definition's last step in float64 on
a given row, and ``frequency_bound`` says how far the device may be from it.

The bound, u = 2^-24, T = float32(2 pi) = 2 pi (1 + dT), |dT| < u / 2:
    re = fmaf(a.x, b.x, a.y * b.y), im = fmaf(a.y, b.x, -(a.x * b.y)): two roundings each, |d re|, |d im| <= 2 u |a| |b| and
        |z| = |a| |b|, so the angle of (re, im) is within 2 sqrt(2) u of the exact product's                   Z_ANGLE
    dphi = atan2f(im, re): within ATAN_GATE of the float64 arctangent of the same (re, im), measured          ATAN_GATE
    num = dphi + T * k: the product rounds once and carries dT (2 u relative to 2 pi |k|), the sum rounds once
    scale = hz / (T * span): the product is exact (span is 1 or 2) and carries dT, the quotient rounds once
    frequency = num * scale: one rounding.  So relative to |dphi + 2 pi k|: 1 (sum) + 1 (dT) + 1 (quotient) + 1 (product)
    |f_dev - f| <= hz / (2 pi span) (Z_ANGLE + ATAN_GATE + 2 u 2 pi |k| + 4 u |dphi + 2 pi k|) (1 + SECOND_ORDER)
where k is the same integer on both sides: it is one unless (span nu - dphi) / (2 pi) lies within K_MARGIN of a half-integer,
where the device's own rounding of that quotient (3 roundings, and the arctangent's error over 2 pi) may take the other
neighbour; there either integer is accepted (``frequency64`` reports the margin).
"""
import numpy as np

from bandpass_model import fmaf32, norm2_32

U = 2.0 ** -24
TWO_PI32 = np.float32(2 * np.pi)
Z_ANGLE = 2 * np.sqrt(2.0) * U
# The device library's atan2f against float64 arctan2 of the same float32 (im, re), on an MI355X, over every frequency
# cell of tests/test_gpu_ridge.py's kernel cases (profiles/ridge.md has the measurement): the worst absolute difference.
ATAN_WORST = 2.871e-7
ATAN_GATE = 2 * ATAN_WORST
assert ATAN_GATE <= 2e-6                                  # 8 ulp of pi: an arctangent that needs more is wrong
SECOND_ORDER = 1e-5
K_MARGIN = 1e-5


def _segments_of_columns(segments, n):
    """(start, stop) of every column's segment, each (n,)."""
    seg = np.asarray(segments, dtype=np.int64).reshape(-1, 2)
    assert seg[0, 0] == 0 and seg[-1, 1] == n and np.all(seg[1:, 0] == seg[:-1, 1]) and np.all(seg[:, 1] > seg[:, 0])
    which = np.searchsorted(seg[:, 0], np.arange(n), side="right") - 1
    return seg[which, 0], seg[which, 1]


def neighbours(segments, n):
    """tm, tp, span of every column."""
    start, stop = _segments_of_columns(segments, n)
    t = np.arange(n)
    tm, tp = np.maximum(t - 1, start), np.minimum(t + 1, stop - 1)
    return tm, tp, tp - tm


def _pick(q, idx):
    return np.take_along_axis(q, idx[:, None, :], axis=1)[:, 0]


def _rank(q, a, cnt):
    """q (C, cnt, n) of the band's rows -> (row, q_win, qm, qp, interior)."""
    idx = np.argmax(q, axis=1)                                             # the first of equal maxima
    qw = _pick(q, idx)
    win = qw > 0
    row = np.where(win, a + idx, -1).astype(np.int32)
    interior = win & (idx > 0) & (idx < cnt - 1)
    qm = _pick(q, np.clip(idx - 1, 0, cnt - 1))
    qp = _pick(q, np.clip(idx + 1, 0, cnt - 1))
    return row, np.where(win, qw, 0).astype(q.dtype), qm, qp, interior


def model(w, bands, e, nu, hz_per_cycle, segments):
    """The definition in float64.  {"row" (C, B, n) int32, "amplitude", "offset", "frequency" float64}."""
    w = np.asarray(w, dtype=np.complex128)
    e = np.asarray(e, dtype=np.float64)
    c, _, n = w.shape
    out = {"row": np.zeros((c, len(bands), n), np.int32), "amplitude": np.zeros((c, len(bands), n)),
           "offset": np.zeros((c, len(bands), n)), "frequency": np.zeros((c, len(bands), n))}
    for k, (a, cnt) in enumerate(bands):
        q = e[None, a:a + cnt, None] * (w[:, a:a + cnt].real ** 2 + w[:, a:a + cnt].imag ** 2)
        row, qw, qm, qp, interior = _rank(q, a, cnt)
        d2 = qm + qp - 2 * qw
        ok = interior & (d2 != 0)
        out["row"][:, k] = row
        out["amplitude"][:, k] = np.sqrt(qw)
        out["offset"][:, k] = np.where(ok, 0.5 * (qm - qp) / np.where(ok, d2, 1.0), 0.0)
    out["frequency"] = frequency64(w, out["row"], nu, hz_per_cycle, segments)["frequency"]
    return out


def q32(w, e):
    """q = e * norm2(w) in the prescribed float32 operations: (C, S, n) float32."""
    return np.asarray(e, dtype=np.float32)[None, :, None] * norm2_32(np.asarray(w, dtype=np.complex64))


def ranking32(w, bands, e):
    """The prescribed float32 sequences, bit for bit, for complex64 w: {"row" int32, "amplitude", "offset" float32}."""
    q = q32(w, e)
    c, _, n = q.shape
    out = {"row": np.zeros((c, len(bands), n), np.int32), "amplitude": np.zeros((c, len(bands), n), np.float32),
           "offset": np.zeros((c, len(bands), n), np.float32)}
    for k, (a, cnt) in enumerate(bands):
        row, qw, qm, qp, interior = _rank(q[:, a:a + cnt], a, cnt)
        d1, s = qm - qp, qm + qp                                            # (float32 arrays: one rounding each)
        d2 = s - np.float32(2) * qw
        ok = interior & (d2 != 0)
        with np.errstate(all="ignore"):
            off = (np.float32(0.5) * d1) / np.where(ok, d2, np.float32(1))
        out["row"][:, k] = row
        out["amplitude"][:, k] = np.sqrt(qw)
        out["offset"][:, k] = np.where(ok, off, np.float32(0))
        assert out["offset"].dtype == np.float32 and d2.dtype == np.float32
    return out


def _on_row(w, row, cols):
    """w[c, row[c, b, t], cols[t]] -> (C, B, n); row -1 reads row 0 (the caller masks it)."""
    c = np.arange(w.shape[0])[:, None, None]
    return w[c, np.maximum(row, 0), cols[None, None, :]]


def product32(w, row, segments):
    """(re, im) float32 (C, B, n): the prescribed fmaf pair of W[row, tp] conj(W[row, tm]), and span (n,)."""
    w = np.asarray(w, dtype=np.complex64)
    tm, tp, span = neighbours(segments, w.shape[-1])
    a, b = _on_row(w, row, tp), _on_row(w, row, tm)
    re = fmaf32(a.real, b.real, a.imag * b.imag)
    im = fmaf32(a.imag, b.real, -(a.real * b.imag))
    return re, im, span


def frequency64(w, row, nu, hz_per_cycle, segments):
    """The definition's last step in float64 on the rows ``row`` (C, B, n): {"frequency" (NaN where the definition says),
    "angle": dphi, "k", "span" (n,), "margin": the distance of (span nu - dphi) / (2 pi) from the nearest half-integer}.
    nu and hz_per_cycle are taken as the float64 values of the float32 they are given to the device as."""
    w = np.asarray(w, dtype=np.complex128)
    nu = np.asarray(nu, dtype=np.float32).astype(np.float64)
    hz = float(np.float32(hz_per_cycle))
    tm, tp, span = neighbours(segments, w.shape[-1])
    z = _on_row(w, row, tp) * np.conj(_on_row(w, row, tm))
    dphi = np.angle(z)
    turns = (span[None, None, :] * nu[np.maximum(row, 0)] - dphi) / (2 * np.pi)
    k = np.rint(turns)
    bad = (row < 0) | (span[None, None, :] == 0) | (z == 0)
    with np.errstate(all="ignore"):
        f = (dphi + 2 * np.pi * k) / (2 * np.pi * span[None, None, :]) * hz
    return {"frequency": np.where(bad, np.nan, f), "angle": dphi, "k": k, "span": span,
            "margin": np.abs(np.abs(turns - np.floor(turns)) - 0.5)}


def frequency_bound(angle, k, span, hz_per_cycle, extra_angle=0.0):
    """|f_dev - f| for a cell whose float64 phase advance is ``angle`` + 2 pi ``k`` over ``span`` columns (the docstring
    above counts it); ``extra_angle``: what else the angle may be off by, e.g. what the transform's gate allows."""
    span = np.asarray(span, dtype=np.float64)
    total = np.abs(np.asarray(angle) + 2 * np.pi * np.asarray(k))
    with np.errstate(all="ignore"):
        return (float(np.float32(hz_per_cycle)) / (2 * np.pi * span)
                * (Z_ANGLE + ATAN_GATE + extra_angle + 2 * U * 2 * np.pi * np.abs(k) + 4 * U * total) * (1 + SECOND_ORDER))


def frequency_error(got, w, row, nu, hz_per_cycle, segments, extra_angle=0.0):
    """The device's ``frequency`` against frequency64 on ``row``: (worst error / bound over the finite cells, the number of
    cells where the unwrapping integer was within K_MARGIN of a tie and either neighbour was accepted).  Asserts that the
    NaNs are exactly the definition's."""
    ref = frequency64(w, row, nu, hz_per_cycle, segments)
    nan = np.isnan(ref["frequency"])
    assert np.array_equal(np.isnan(got), nan), int(np.count_nonzero(np.isnan(got) != nan))
    span = np.broadcast_to(ref["span"][None, None, :], got.shape)
    live = ~nan
    hz = float(np.float32(hz_per_cycle))
    extra = np.broadcast_to(np.asarray(extra_angle, dtype=np.float64), got.shape)
    loose = live & (ref["margin"] <= K_MARGIN + extra / (2 * np.pi))
    err = np.abs(got.astype(np.float64) - ref["frequency"])
    step = hz / np.where(span > 0, span, 1)
    err = np.where(loose, np.minimum(err, np.minimum(np.abs(err - step), np.abs(err + step))), err)
    k = np.where(loose, np.abs(ref["k"]) + 1, ref["k"])
    bound = frequency_bound(ref["angle"], k, np.where(span > 0, span, 1), hz, extra)
    ratio = (err[live] / bound[live]).max(initial=0.0)
    return float(ratio), int(np.count_nonzero(loose))


CHIRP_FREQS = np.geomspace(20.0, 100.0, 19)                # the rows the chirp is followed on: 8.2 per octave, ascending


def chirp(n=12000, fs=1000.0, f0=31.0, f1=67.0, amplitude=0.8):
    """The chirp the ridge is followed on end to end: a linear sweep f0 -> f1 Hz over the recording."""
    t = np.arange(n) / fs
    return amplitude * np.cos(2 * np.pi * (f0 * t + 0.5 * (f1 - f0) / (n / fs) * t * t) + 0.4)


def near_ties(q, bands, rel=4e-5):
    """(C, B, n) bool: the columns whose two largest q of a band lie within ``rel`` of each other, relative to the largest
    (a band of one row has none)."""
    out = np.zeros((q.shape[0], len(bands), q.shape[-1]), bool)
    for k, (a, cnt) in enumerate(bands):
        if cnt < 2:
            continue
        top = np.sort(q[:, a:a + cnt], axis=1)[:, -2:]
        out[:, k] = (top[:, 1] - top[:, 0]) <= rel * top[:, 1]
    return out
