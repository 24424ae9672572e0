"""NumPy twin of the definition of gcwt_trace_smooth (include/ghostcwt.h) and of the pieces detect(smooth=, combine=) adds.

Combine is a chain of float32 additions in the order of the list and one float32 product: NumPy's float32 scalars round
each once, so the model is the answer, bit for bit.  The smoother is a chain of float32 operations whose order the device
prescribes; the model convolves in float64 with the same float32 taps and derives, from the data, how far the chain may
lie from it.  u = 2^-24, gamma_m = m u / (1 - m u).  Per output column, with p_k = v[c - k] + v[c + k]:
    acc_0 = fl(w_0 v[c])                                  one rounding
    acc_k = fl(w_k fl(p_k) + acc_(k-1)),  k = 1 .. half   two roundings: the pair's addition and the fused multiply-add
so the term of tap k passes through its pair's addition, its own fused multiply-add and the half - k later ones: half - k +
2 <= half + 1 roundings for k >= 1, and half + 1 for k = 0.  Each factor (1 + d), |d| <= u, and |p_k| <= |v[c - k]| + |v[c +
k]| give
    |out - exact| <= gamma_(half + 1) sum_k w_k (|v[c - k]| + |v[c + k]|)        (k = 0: w_0 |v[c]| once; taps >= 0)
the standard bound of a recursive sum (Higham, Accuracy and Stability of Numerical Algorithms, lemma 3.1 and section 4.2).
The model's own float64 convolution of 2 half + 1 terms adds gamma64_(2 half + 2) of the same sum.  Nothing here is
measured."""
import numpy as np

U = 2.0 ** -24
U64 = 2.0 ** -53


def gamma(m, u=U):
    return m * u / (1 - m * u)


def taps(sd_cols):
    """engine.smooth_taps' definition: half = int(4 sd + 0.5), Gaussian weights normalised in float64, rounded once."""
    half = int(4 * sd_cols + 0.5)
    k = np.arange(half + 1, dtype=np.float64)
    w = np.exp(-0.5 * (k / sd_cols) ** 2)
    return (w / (w[0] + 2 * w[1:].sum())).astype(np.float32)


def taps_of_half(half):
    """Gaussian taps that reach exactly ``half`` columns (sd = half / 4), for kernels of a given length; [1] for half = 0."""
    if half == 0:
        return np.ones(1, np.float32)
    k = np.arange(half + 1, dtype=np.float64)
    w = np.exp(-0.5 * (k / (half / 4.0)) ** 2)
    return (w / (w[0] + 2 * w[1:].sum())).astype(np.float32)


def combine(traces, members):
    """The mean trace, bit for bit: s = v[m_0]; s = s + v[m_i] in the order of the list; s * float32(1.0 / M)."""
    traces = np.asarray(traces, dtype=np.float32)
    members = [int(m) for m in members]
    with np.errstate(all="ignore"):
        s = traces[members[0]].copy()
        for m in members[1:]:
            s = (s + traces[m]).astype(np.float32)                          # float32 + float32: one rounding
        return (s * np.float32(1.0 / len(members))).astype(np.float32)


def _whole(n):
    return np.array([[0, n]], dtype=np.int64)


def _kernel(w):
    w = np.asarray(w, dtype=np.float32).astype(np.float64)
    return np.concatenate((w[:0:-1], w))                                    # w_half .. w_1, w_0, w_1 .. w_half


def smooth(trace, w, segments=None):
    """One trace (n,) float32 -> float64 (n,): every segment convolved on its own with zeros past its ends, a column in no
    segment 0.  A NaN reaches the columns within half of it inside its segment and no others."""
    v = np.asarray(trace, dtype=np.float32).astype(np.float64)
    kern, half = _kernel(w), len(w) - 1
    out = np.zeros(v.size)
    with np.errstate(all="ignore"):
        for a, b in (_whole(v.size) if segments is None else np.asarray(segments)):
            out[a:b] = np.convolve(v[a:b], kern)[half:half + (b - a)]
    return out


def bound(trace, w, segments=None):
    """(n,) float64: how far the device's float32 chain may lie from smooth() -- the derived bound plus the model's own
    float64 rounding.  NaN / inf where the trace's window holds one."""
    v = np.abs(np.asarray(trace, dtype=np.float32).astype(np.float64))
    kern, half = np.abs(_kernel(w)), len(w) - 1
    out = np.zeros(v.size)
    with np.errstate(all="ignore"):
        for a, b in (_whole(v.size) if segments is None else np.asarray(segments)):
            out[a:b] = np.convolve(v[a:b], kern)[half:half + (b - a)]
        return (gamma(half + 1) + gamma(2 * half + 2, U64)) * out


def reach(where, half, n, segments=None):
    """bool (n,): the columns within ``half`` of a column of ``where`` (bool (n,)) inside the same segment."""
    out = np.zeros(n, bool)
    for a, b in (_whole(n) if segments is None else np.asarray(segments)):
        for c in np.flatnonzero(where[a:b]) + a:
            out[max(a, c - half):min(b, c + half + 1)] = True
    return out


def segments_of(time, period, fs, n_cols):
    """engine.segments_of's rule as a plain loop: a boundary before column j where |t[j] - t[j - 1] - period| > 0.5 / fs."""
    if time is None:
        return _whole(n_cols)
    starts = [0]
    for j in range(1, n_cols):
        if abs(time[j] - time[j - 1] - period) > 0.5 / fs:
            starts.append(j)
    return np.array([[a, b] for a, b in zip(starts, starts[1:] + [n_cols])], dtype=np.int64)
