"""Float64 NumPy twin of gcwt_triggered's definition (include/ghostcwt.h): event-locked averages of complex rows.

W (C, S, n_cols) complex; event columns e_0 .. e_{E-1}; nb columns before and na after, L = nb + na + 1 lags, lag l
standing for column e_k - nb + l.  For a channel c, a row r and a lag l, with w_k = W[c, r, e_k - nb + l]:
    a_k = |w_k|,   u_k = w_k / |w_k| (0 where that is 0),
    amplitude = sum a_k / E,   power = sum a_k^2 / E,   evoked = sum w_k / E,   vector = sum u_k / E,
    itpc = |sum u_k| / E.

The bounds below are derived from the order csrc/triggered.hip prescribes, not measured.  u = 2^-24, n = ceil(E / 4).
"""
import numpy as np

U = 2.0 ** -24

# Roundings a term carries when it enters its chain, each relative to the term (every operation is a single correctly
# rounded float32 one):
#   r2 = fmaf(im, im, re * re)    2                                   -> the term of `power` carries 2
#   a = sqrt(r2)                  the root halves r2's two, adds 1    -> the term of `amplitude` carries 2
#   inv = 1 / a                   1
#   u = (re * inv, im * inv)      1                                   -> a component of `vector`'s term: 2 + 1 + 1 = 4
#   w = (re, im)                  0: the rows themselves              -> a component of `evoked`'s term carries 0
K_AMPLITUDE, K_POWER, K_EVOKED, K_VECTOR = 2, 2, 0, 4


def chain(n_events):
    """n: the events one of the four interleaved chains adds one after the other."""
    return -(-int(n_events) // 4)


def _sum_roundings(n_events):
    """The chain of ceil(E / 4) adds, 2 for the combination (X0 + X1) + (X2 + X3), 1 for the divide by E."""
    return chain(n_events) + 2 + 1


def amplitude_bound(n_events):
    """Relative to amplitude (all terms are >= 0, so every partial sum is at most the whole)."""
    return (K_AMPLITUDE + _sum_roundings(n_events)) * U


def power_bound(n_events):
    """Relative to power."""
    return (K_POWER + _sum_roundings(n_events)) * U


def evoked_bound(n_events):
    """|evoked_dev - evoked_ref| relative to amplitude = sum |w_k| / E, which bounds the sum of |re_k| and of |im_k|
    and every partial sum of a component; sqrt(2) for the two components."""
    return np.sqrt(2.0) * (K_EVOKED + _sum_roundings(n_events)) * U


def vector_bound(n_events):
    """|vector_dev - vector_ref|, absolute: sum |u_k.x| / E <= 1; sqrt(2) for the two components."""
    return np.sqrt(2.0) * (K_VECTOR + _sum_roundings(n_events)) * U


def itpc_bound(n_events):
    """|V| / E <= 1: the vector's error, and 3 more: the modulus' two roundings halved by the root, the root, and the
    divide (the min with 1 only moves a value towards the reference, which is at most 1)."""
    return vector_bound(n_events) + 3 * U


def unit(w):
    """w / |w|, 0 where |w| == 0."""
    w = np.asarray(w, dtype=np.complex128)
    r = np.abs(w)
    return np.where(r > 0, w / np.where(r > 0, r, 1.0), 0.0)


def windows(w, cols, nb, na, rows=None):
    """(C, R, E, L) complex128: the window of every event out of the rows (first, count) = ``rows`` (None: all)."""
    w = np.asarray(w)
    cols = np.asarray(cols, dtype=np.int64)
    first, count = (0, w.shape[1]) if rows is None else rows
    idx = cols[:, None] - nb + np.arange(nb + na + 1)[None, :]
    assert idx.min() >= 0 and idx.max() < w.shape[-1], "a window leaves the columns"
    return w[:, first:first + count][:, :, idx].astype(np.complex128)


def model(w, cols, nb, na, rows=None):
    """{"amplitude", "power", "itpc" (C, R, L) float64, "evoked", "vector" (C, R, L) complex128}."""
    seg = windows(w, cols, nb, na, rows)
    n_events = seg.shape[2]
    amp = np.abs(seg)
    vec = unit(seg).sum(axis=2)
    return {"amplitude": amp.sum(axis=2) / n_events, "power": (amp * amp).sum(axis=2) / n_events,
            "evoked": seg.sum(axis=2) / n_events, "vector": vec / n_events,
            "itpc": np.minimum(np.abs(vec) / n_events, 1.0)}


def gate_bound(w_ref, cols, nb, na, rows=None):
    """How far each output may move when every coefficient of the float64 reference w_ref (C, S, n) moves by the
    project's gate, eps_r = 1e-5 max_t |W[c, r]| per sample: |w| and w by at most eps, |w|^2 by at most 2 |w| eps +
    eps^2, and a unit phasor turns by at most min(2, 2 eps / |w|).  {"amplitude", "power", "evoked", "vector", "itpc"}:
    (C, R, L), absolute."""
    w_ref = np.asarray(w_ref, dtype=np.complex128)
    first, count = (0, w_ref.shape[1]) if rows is None else rows
    eps = 1e-5 * np.abs(w_ref[:, first:first + count]).max(axis=-1)[..., None]    # C, R, 1
    amp = np.abs(windows(w_ref, cols, nb, na, rows))                            # C, R, E, L
    turn = np.minimum(2.0, 2 * eps[..., None] / np.maximum(amp, 1e-300)).mean(axis=2)
    flat = np.broadcast_to(eps, turn.shape)
    return {"amplitude": flat, "evoked": flat, "power": 2 * eps * amp.mean(axis=2) + eps * eps, "vector": turn, "itpc": turn}


def evoked_input(n=32768, fs=1000.0):
    """-> (x (2, n), events (60,) seconds).  rng 7: two channels of 0.2 * white noise; 60 events from 0.7 s, spaced
    0.4 + 0.1 * rng.random() s, rounded to whole samples, none within 0.7 s of the end; after each event a 40 Hz burst
    exp(-((t - e - 0.1) / 0.03)^2 / 2) * cos(2 pi 40 (t - e) + phi) -- phi = -1.0 in channel 0 (phase-locked), phi drawn
    per event from uniform(0, 2 pi) in channel 1 (induced: the same amplitude, no common phase)."""
    rng = np.random.default_rng(7)
    t = np.arange(n) / fs
    x = 0.2 * rng.standard_normal((2, n))
    events = np.round((0.7 + np.concatenate([[0.0], np.cumsum(0.4 + 0.1 * rng.random(59))])) * fs) / fs
    assert events.size == 60 and events[-1] <= (n - 1) / fs - 0.7
    phi = np.stack([np.full(60, -1.0), rng.uniform(0.0, 2 * np.pi, 60)])
    for ch in range(2):
        for e, p in zip(events, phi[ch]):
            x[ch] += np.exp(-((t - e - 0.1) / 0.03) ** 2 / 2) * np.cos(2 * np.pi * 40 * (t - e) + p)
    return x, events


def check_physics(m, f, nb, fs, stride=1):
    """The asserts on evoked_input's averages (arrays (2, 23, L)): channel 0 is phase-locked at -1.0 rad, channel 1 has
    the same amplitude and no common phase."""
    r = int(np.argmin(np.abs(f - 40.0)))
    at = nb + int(round(0.1 * fs / stride))                                     # lag +100 ms
    base = slice(0, nb - int(round(0.05 * fs / stride)) + 1)                    # lags -200 .. -50 ms
    itpc0, ang0 = float(m["itpc"][0, r, at]), float(np.angle(m["vector"][0, r, at]))
    itpc1, ev1 = float(m["itpc"][1, r].max()), float(abs(m["evoked"][1, r, at]))
    amp = m["amplitude"][:, r, at]
    rest = m["amplitude"][:, r, base].mean(axis=-1)
    print("row %.1f Hz, lag +100 ms: channel 0 itpc %.4f angle %.3f rad; channel 1 max itpc %.3f |evoked| %.4f; amplitude %s, "
          "baseline %s" % (f[r], itpc0, ang0, itpc1, ev1, amp, rest))
    assert itpc0 >= 0.95
    assert abs(ang0 - (-1.0)) <= 0.25
    assert itpc1 <= 0.35
    assert ev1 <= 0.2 * amp[1]
    assert np.all(amp >= 10 * rest)
