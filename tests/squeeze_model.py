"""NumPy twins of gcwt_squeeze's definition (include/ghostcwt.h): the synchrosqueezed transform of a run of rows.

W (C, S, n_cols) complex; the input rows are first .. first + R - 1; g, floor2 >= 0, nu >= 0: (S,) tables; segments (n, 2) of
(start, stop) covering [0, n_cols); edges (L + 1,) float32, > 0, strictly ascending.  For a channel c, an input row r and a
column t, with w = W[c, r, t]:
    frequency[c, r - first, t] = ridge_model's frequency on row r (the phase advance between the neighbouring columns of the
        same segment, unwrapped against nu_r); NaN where the span is 0 or the product is 0
    the entry is out where !(norm2(w) > floor2_r), frequency is NaN, frequency < edges[0] or frequency >= edges[L]; else its cell
        is the largest l with edges[l] <= frequency
    index[c, r - first, t] = l, or L - 1 - l with ``descending``; -1 where the entry is out
    coefficients[c, row, t] = sum of g_r w over the entries with index == row, the rows in ascending r;  power = |coefficients|^2

Two models.  ``model`` is the definition in float64 -- but for the threshold, which the definition itself puts on the float32
``norm2`` (bandpass_model.norm2_32) of the complex64 coefficient: that comparison is exact, so the model makes it on the same
number.  ``index32`` and ``chain32`` are the prescribed float32 steps themselves, bit for bit: the cell of a given float32
frequency (np.searchsorted on the float32 edges is the binary search's answer), and the chain of fused multiply-adds *given an
index map* -- the arctangent in ``frequency`` is the device library's and is not modelled, so the device's own index is what
its sums are held to.

Where the float64 model may name another cell than the device (``undecidable``): where its frequency lies within
ridge_model.frequency_bound of an edge -- the device's frequency is only that close to it --, and where the unwrapping integer
was within ridge_model.K_MARGIN of a tie, so that the device's frequency may be one whole turn away (ridge_model accepts
either neighbour there, too).  Everywhere else the two indices must agree.
"""
import numpy as np

import ridge_model as rm
from bandpass_model import fmaf32, norm2_32


def every_row(first, count, c, n):
    """The (C, R, n) row map that ridge_model's functions take: row first + j on plane j."""
    return np.broadcast_to(np.arange(first, first + count, dtype=np.int32)[None, :, None], (c, count, n))


def cells_of(frequency, inside, edges, descending):
    """The definition's cell rule on given frequencies (any float dtype; compared as they are with the float32 edges'
    values): int32 output rows, -1 where ``inside`` is False, the frequency is NaN, < edges[0] or >= edges[L]."""
    edges = np.asarray(edges, dtype=np.float32)
    n_cells = edges.size - 1
    f = np.asarray(frequency)
    with np.errstate(invalid="ignore"):
        ok = inside & ~np.isnan(f) & (f >= edges[0]) & (f < edges[-1])
    cell = np.searchsorted(edges.astype(f.dtype), np.where(ok, f, edges[0].astype(f.dtype)), side="right") - 1
    row = n_cells - 1 - cell if descending else cell
    return np.where(ok, row, -1).astype(np.int32)


def inside32(w, rows, floor2):
    """norm2(w) > floor2_r in the prescribed float32 operations: (C, R, n) bool."""
    first, count = rows
    w = np.asarray(w, dtype=np.complex64)[:, first:first + count]
    return norm2_32(w) > np.asarray(floor2, dtype=np.float32)[None, first:first + count, None]


def index32(frequency32, w, rows, floor2, edges, descending):
    """The index that the definition derives from a given float32 ``frequency`` plane (C, R, n) -- the device's own --, bit
    for bit."""
    assert frequency32.dtype == np.float32
    return cells_of(frequency32, inside32(w, rows, floor2), edges, descending)


def chain32(w, rows, g, index, n_cells):
    """The prescribed float32 chain over a given index map (C, R, n), bit for bit, for complex64 w: {"coefficients" (C, L, n)
    complex64, "power" float32}.  One rounding per fused multiply-add, the rows in ascending order, from exact zeros."""
    first, count = rows
    w = np.asarray(w, dtype=np.complex64)
    g = np.asarray(g, dtype=np.float32)
    c, _, n = w.shape
    re, im = np.zeros((c, n_cells, n), np.float32), np.zeros((c, n_cells, n), np.float32)
    for j in range(count):
        ci, ti = np.nonzero(index[:, j] >= 0)
        at = (ci, index[ci, j, ti], ti)
        wr = w[ci, first + j, ti]
        re[at] = fmaf32(g[first + j], wr.real, re[at])
        im[at] = fmaf32(g[first + j], wr.imag, im[at])
    z = (re + 1j * im).astype(np.complex64)
    return {"coefficients": z, "power": norm2_32(z)}


def sums64(w, rows, g, index, n_cells):
    """The same sums in float64 over a given index map: (C, L, n) complex128."""
    first, count = rows
    w = np.asarray(w, dtype=np.complex128)
    g = np.asarray(g, dtype=np.float64)
    c, _, n = w.shape
    z = np.zeros((c, n_cells, n), np.complex128)
    for j in range(count):
        ci, ti = np.nonzero(index[:, j] >= 0)
        at = (ci, index[ci, j, ti], ti)
        z[at] += g[first + j] * w[ci, first + j, ti]
    return z


def model(w, rows, g, floor2, nu, hz_per_cycle, segments, edges, descending, inside=None, extra_angle=0.0):
    """The definition in float64.  ``inside``: the (C, R, n) threshold mask, default inside32 of complex64(w).  -> {"frequency"
    (C, R, n) float64, "index" int32, "coefficients" (C, L, n) complex128, "power", "bound": how far the device's frequency may
    be from "frequency" (ridge_model.frequency_bound, ``extra_angle`` as there), "undecidable": (C, R, n) bool, see the
    module's docstring, "inside"}."""
    first, count = rows
    w = np.asarray(w, dtype=np.complex128)
    c, _, n = w.shape
    edges = np.asarray(edges, dtype=np.float32)
    if inside is None:
        inside = inside32(w, rows, floor2)
    ref = rm.frequency64(w, every_row(first, count, c, n), nu, hz_per_cycle, segments)
    f = ref["frequency"]
    index = cells_of(f, inside, edges, descending)
    span = np.broadcast_to(ref["span"][None, None, :], f.shape)
    extra = np.broadcast_to(np.asarray(extra_angle, dtype=np.float64), f.shape)
    bound = rm.frequency_bound(ref["angle"], ref["k"], np.where(span > 0, span, 1), hz_per_cycle, extra)
    live = ~np.isnan(f)
    with np.errstate(invalid="ignore"):
        nearest = np.abs(np.where(live, f, 0.0)[..., None] - edges.astype(np.float64)).min(axis=-1)
        undecidable = live & ((nearest <= bound) | (ref["margin"] <= rm.K_MARGIN + extra / (2 * np.pi)))
    z = sums64(w, rows, g, index, edges.size - 1)
    return {"frequency": f, "index": index, "coefficients": z, "power": np.abs(z) ** 2, "bound": bound,
            "undecidable": undecidable, "inside": inside}


def brute(w, rows, g, floor2, nu, hz_per_cycle, segments, edges, descending):
    """The definition once more, entry by entry in plain Python loops (float64; the threshold on the float32 norm2): what
    ``model`` is checked against on small inputs.  -> (frequency, index, coefficients)."""
    first, count = rows
    w64 = np.asarray(w, dtype=np.complex128)
    r2 = norm2_32(np.asarray(w, dtype=np.complex64))
    nu = np.asarray(nu, dtype=np.float32).astype(np.float64)
    floor2 = np.asarray(floor2, dtype=np.float32)
    hz = float(np.float32(hz_per_cycle))
    e = [float(v) for v in np.asarray(edges, dtype=np.float32)]
    n_cells = len(e) - 1
    c, _, n = w64.shape
    freq = np.full((c, count, n), np.nan)
    index = np.full((c, count, n), -1, np.int32)
    z = np.zeros((c, n_cells, n), np.complex128)
    for start, stop in np.asarray(segments).reshape(-1, 2):
        for t in range(start, stop):
            tm, tp = max(t - 1, start), min(t + 1, stop - 1)
            for ch in range(c):
                for j in range(count):
                    r = first + j
                    prod = w64[ch, r, tp] * np.conj(w64[ch, r, tm])
                    if tp > tm and prod != 0:
                        dphi = np.angle(prod)
                        k = np.rint(((tp - tm) * nu[r] - dphi) / (2 * np.pi))
                        freq[ch, j, t] = (dphi + 2 * np.pi * k) / (2 * np.pi * (tp - tm)) * hz
                    f = freq[ch, j, t]
                    if not r2[ch, r, t] > floor2[r] or np.isnan(f) or f < e[0] or f >= e[-1]:
                        continue
                    cell = max(l for l in range(n_cells) if e[l] <= f)
                    index[ch, j, t] = n_cells - 1 - cell if descending else cell
                    z[ch, index[ch, j, t], t] += float(np.float32(g[r])) * w64[ch, r, t]
    return freq, index, z


def frequency_error(got, w, rows, nu, hz_per_cycle, segments, where, extra_angle=0.0):
    """ridge_model.frequency_error on every row, held to the entries ``where`` (C, R, n) only -- the NaNs must be the
    definition's there, and the worst error / bound is taken there -> (ratio, cells whose unwrapping integer was a tie)."""
    first, count = rows
    c, _, n = np.shape(w)
    ref = rm.frequency64(w, every_row(first, count, c, n), nu, hz_per_cycle, segments)
    nan = np.isnan(ref["frequency"])
    assert np.array_equal(np.isnan(got)[where], nan[where]), int(np.count_nonzero((np.isnan(got) != nan) & where))
    span = np.broadcast_to(ref["span"][None, None, :], got.shape)
    live = ~nan & where
    hz = float(np.float32(hz_per_cycle))
    extra = np.broadcast_to(np.asarray(extra_angle, dtype=np.float64), got.shape)
    loose = live & (ref["margin"] <= rm.K_MARGIN + extra / (2 * np.pi))
    with np.errstate(invalid="ignore"):
        err = np.abs(got.astype(np.float64) - ref["frequency"])
        step = hz / np.where(span > 0, span, 1)
        err = np.where(loose, np.minimum(err, np.minimum(np.abs(err - step), np.abs(err + step))), err)
    k = np.where(loose, np.abs(ref["k"]) + 1, ref["k"])
    bound = rm.frequency_bound(ref["angle"], k, np.where(span > 0, span, 1), hz, extra)
    return float((err[live] / bound[live]).max(initial=0.0)), int(np.count_nonzero(loose))


# -- the end-to-end case: tests/ridge_model.py's chirp, 38 cells, a threshold at 5 % of its amplitude ---------------------------
BINS = 38
MIN_AMPLITUDE = 0.04
UNDECIDABLE_CAP = 0.02                                      # of the entries above the threshold


FS = 1000.0
_CACHE = {}


def chirp_case(kind, stride):
    """The end-to-end case on the oracle alone, made once per (kind, stride) and shared, read-only: the two-channel chirp of
    tests/test_gpu_ridge.py on ridge_model.CHIRP_FREQS, ``kind`` 'morse' (the default wavelet, against ghost_oracle) or 'morlet'
    (Morlet(6), against morlet_cases.truth), every ``stride``-th column; BINS cells between the rows' end frequencies.  ->
    {"x", "f", "wavelet", "ref_w" (2, S, N), "e", "g", "h", "centres", "edges", "descending", "segments", "n", "model":
    oracle_case's dict}."""
    key = (kind, stride)
    if key not in _CACHE:
        from ghost_amd import engine
        from ghost_amd.wave import Morlet
        from ghost_amd.wave.morse import Morse
        import morlet_cases
        from oracle import ghost_oracle as orc
        x = np.stack([rm.chirp(), 0.5 * rm.chirp()[::-1]])
        f = rm.CHIRP_FREQS
        if kind == "morlet":
            wavelet = Morlet(w0=6.0, fs=FS)
            full = np.stack([morlet_cases.truth(x[ch], FS, f, 6.0) for ch in range(2)])
        else:
            wavelet = Morse(fs=FS, gamma=3.0, beta=20.0)
            full = np.stack([orc.cwt_complex(x[ch], FS, f) for ch in range(2)])
        ref_w = np.ascontiguousarray(full[..., ::stride])
        n = ref_w.shape[-1]
        g, h = engine.band_weights(f, wavelet)
        e = engine.ridge_weights(f, wavelet)
        centres = np.geomspace(f[0], f[-1], BINS)
        edges, descending = engine.squeeze_edges(centres)
        segments = np.array([[0, n]], dtype=np.int64)
        case = {"x": x, "f": f, "wavelet": wavelet, "ref_w": ref_w, "e": e, "g": g, "h": h, "centres": centres, "edges": edges,
                "descending": descending, "segments": segments, "n": n,
                "model": oracle_case(ref_w, f, (0, f.size), e, g, stride, FS, segments, edges, descending)}
        for v in list(case.values()) + list(case["model"].values()):
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CACHE[key] = case
    return _CACHE[key]


def chirp_frequency(n_samples, stride):
    """The instantaneous frequency of ridge_model.chirp() at every ``stride``-th sample (channel 0; channel 1 is its mirror)."""
    return (31.0 + (67.0 - 31.0) * np.arange(n_samples) / n_samples)[::stride]


def concentration(power, centres_or_rows, inst, mid, reach=1):
    """The share of ``power`` (L, n) over the columns ``mid`` that lies within ``reach`` planes of the plane whose frequency
    (``centres_or_rows`` (L,), ascending) is nearest in ln f to the true frequency ``inst`` (n,)."""
    lnf = np.log(np.asarray(centres_or_rows, dtype=np.float64))
    true = np.abs(lnf[:, None] - np.log(inst)[None, :]).argmin(axis=0)
    near = np.abs(np.arange(lnf.size)[:, None] - true[None, :]) <= reach
    p = np.asarray(power, dtype=np.float64)
    return float((p * near)[:, mid].sum() / p[:, mid].sum())


def gate_angle(ref_w, rows):
    """What the transform's gate -- eps_r = 1e-5 max_t |W_r| on every sample of row r -- allows the phase advance of every
    entry to move by: asin(eps_r / |a|) + asin(eps_r / |b|) for the two neighbours a, b (pi where that has no meaning), as
    test_gpu_ridge.py builds it.  Needs the segments only through the caller's neighbours: -> a function of (tm, tp)."""
    first, count = rows
    mag = np.abs(np.asarray(ref_w)[:, first:first + count])
    eps = 1e-5 * mag.max(axis=-1, keepdims=True)

    def at(tm, tp):
        with np.errstate(all="ignore"):
            extra = np.arcsin(np.minimum(eps / mag[..., tp], 1)) + np.arcsin(np.minimum(eps / mag[..., tm], 1))
        return np.where(np.isfinite(extra), extra, np.pi)
    return at


def oracle_case(ref_w, f, rows, e, g, stride, fs, segments, edges, descending, min_amplitude=MIN_AMPLITUDE):
    """The float64 model on the oracle's coefficients ref_w (C, S, N) with what the gate allows: -> the model's dict plus
    "above": the entries whose modulus is above the threshold, "decidable": above or below the threshold by more than the
    gate's eps_r and with a frequency farther from every edge than its bound, "extra": the gate's angle."""
    first, count = rows
    ref_w = np.asarray(ref_w, dtype=np.complex128)
    n = ref_w.shape[-1]
    nu, hz = 2 * np.pi * np.asarray(f) * stride / fs, fs / stride
    tm, tp, _ = rm.neighbours(segments, n)
    extra = gate_angle(ref_w, rows)(tm, tp)
    mag = np.abs(ref_w[:, first:first + count])
    threshold = (min_amplitude / np.sqrt(np.asarray(e, dtype=np.float64)))[None, first:first + count, None]
    above = mag > threshold
    floor2 = (min_amplitude ** 2 / np.asarray(e, dtype=np.float64)).astype(np.float32)
    out = model(ref_w, rows, g, floor2, nu, hz, segments, edges, descending, inside=above, extra_angle=extra)
    eps = 1e-5 * mag.max(axis=-1, keepdims=True)
    out.update(above=above, extra=extra, floor2=floor2, nu=nu, hz=hz,
               decidable=~out["undecidable"] & (np.abs(mag - threshold) > eps))
    return out
