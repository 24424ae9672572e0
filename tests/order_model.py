"""NumPy twin of the definition of gcwt_trace_order (include/ghostcwt.h) and of engine.trace_median_mad.

Everything the entry returns is an integer, a copy of an input value or of one float32 subtraction, so the model is the
answer, bit for bit: the included columns (v != 0, a NaN included), their keys (v, or |v - center| in float32), a stable
argsort of ord(key), the rank-th key.  Nothing here is measured."""
import numpy as np

NO_VALUE = np.array([0x7fc00000], np.uint32).view(np.float32)[0]           # what a rank >= n returns
MAD_TO_SD = 1.482602218505602


def ord(key):
    """uint32 whose unsigned order is the total order of the float32 keys: -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN."""
    u = np.ascontiguousarray(key, dtype=np.float32).view(np.uint32)
    return u ^ np.where(u >> np.uint32(31), np.uint32(0xffffffff), np.uint32(0x80000000))


def keys(trace, center=None):
    """The keys of the included columns of one trace, in column order (float32)."""
    v = np.ascontiguousarray(trace, dtype=np.float32).ravel()
    with np.errstate(invalid="ignore"):
        v = v[v != 0]                                                       # both zeros out, a NaN in
        if center is None:
            return v
        return np.abs(v - np.float32(center))                               # one float32 subtraction; |.| clears the sign bit


def model_order(traces, ranks, center=None):
    """traces (C, n) float32; ranks (C, R) or (R,), 0-based; center None or (C,) -> (n (C,) int64, values (C, R) float32)."""
    traces = np.atleast_2d(np.asarray(traces, dtype=np.float32))
    c = traces.shape[0]
    ranks = np.asarray(ranks, dtype=np.int64)
    ranks = np.broadcast_to(ranks, (c, ranks.shape[-1]))
    n, values = np.zeros(c, np.int64), np.full(ranks.shape, NO_VALUE, np.float32)
    for i in range(c):
        k = keys(traces[i], None if center is None else np.asarray(center, dtype=np.float32)[i])
        k = k[np.argsort(ord(k), kind="stable")]
        n[i] = k.size
        for j, r in enumerate(ranks[i]):
            if 0 <= r < k.size:
                values[i, j] = k[r]
    return n, values


def model_median_mad(traces):
    """(n int64, median float64, mad float64) per trace as engine.trace_median_mad prescribes them: the mean of the ranks
    (n - 1) // 2 and n // 2 in float64 (exact); the same ranks of |v - float32(median)| in float32; both 0 where n == 0 (and
    mad NaN where the median is not finite: there is no centre to subtract)."""
    traces = np.atleast_2d(np.asarray(traces, dtype=np.float32))
    c = traces.shape[0]
    n, median, mad = np.zeros(c, np.int64), np.zeros(c), np.zeros(c)
    for i in range(c):
        k = keys(traces[i])
        n[i] = k.size
        if k.size == 0:
            continue
        lo, hi = (k.size - 1) // 2, k.size // 2
        s = k[np.argsort(ord(k), kind="stable")]
        with np.errstate(invalid="ignore"):
            median[i] = (np.float64(s[lo]) + np.float64(s[hi])) / 2
        if not np.isfinite(median[i]):
            mad[i] = np.nan
            continue
        d = keys(traces[i], np.float32(median[i]))
        d = d[np.argsort(ord(d), kind="stable")]
        with np.errstate(invalid="ignore"):
            mad[i] = (np.float64(d[lo]) + np.float64(d[hi])) / 2
    return n, median, mad
