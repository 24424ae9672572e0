"""NumPy twin of the definitions of gcwt_trace_runs and gcwt_trace_stats (include/ghostcwt.h) and of detect()'s event list.

The runs are exact -- integers and copies of input values -- so the model is the answer, bit for bit.  The statistics are
float64 sums in an order the device prescribes; the model sums with math.fsum (correctly rounded) and derives, from the data,
what any order of summation may differ by.  u = 2^-53, n terms, gamma_n = n u / (1 - n u):
    |s1 - exact| <= gamma_n sum |v|        |s2 - exact| <= gamma_n sum v^2        (v * v is exact in float64)
(adding an exact 0 costs nothing, so n counts the non-zero columns alone), carried through mean = s1 / n and sd =
sqrt(max(s2 / n - mean^2, 0)) one rounding at a time in `_propagate`.  Nothing here is measured."""
import math

import numpy as np

U = 2.0 ** -53


def above(v, lo):
    """Strictly above: a NaN is not."""
    with np.errstate(invalid="ignore"):
        return np.asarray(v) > lo


def model_runs(traces, lo):
    """traces (C, n) float32, lo (C,) -> dict of trace, start, stop, peak_col (int64), peak (float32) over the runs, ordered by
    trace and then by start, and counts (C,)."""
    traces = np.atleast_2d(np.asarray(traces, dtype=np.float32))
    lo = np.broadcast_to(np.asarray(lo, dtype=np.float32), (traces.shape[0],))
    out = {k: [] for k in ("trace", "start", "stop", "peak_col", "peak")}
    counts = np.zeros(traces.shape[0], np.int64)
    for i, v in enumerate(traces):
        edge = np.diff(np.concatenate(([0], above(v, lo[i]).astype(np.int8), [0])))
        starts, stops = np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)
        counts[i] = starts.size
        for a, b in zip(starts, stops):
            at = a + int(np.argmax(v[a:b]))                                 # the first of equal maxima
            out["trace"].append(i), out["start"].append(a), out["stop"].append(b), out["peak_col"].append(at), out["peak"].append(v[at])
    res = {k: np.array(out[k], dtype=np.int64) for k in ("trace", "start", "stop", "peak_col")}
    res["peak"] = np.array(out["peak"], dtype=np.float32)
    res["counts"] = counts
    return res


def model_stats(trace):
    """(n, mean, sd) of one trace over its columns that are not exactly 0, the sums correctly rounded."""
    v = np.asarray(trace, dtype=np.float64).ravel()
    v = v[v != 0]
    n = int(v.size)
    if n == 0:
        return 0, 0.0, 0.0
    mean = math.fsum(v) / n
    return n, mean, math.sqrt(max(math.fsum(v * v) / n - mean * mean, 0.0))


def _propagate(n, sum_abs, q, mean, g):
    """How far mean and sd may lie from their exact values when each sum carries a relative error g of its absolute sum and every
    later operation rounds once: (bound on mean, bound on sd).  q = sum v^2 / n."""
    m = abs(mean)
    bm = g * sum_abs / n + U * m                                            # the sum, then the division
    bq = g * q + U * q
    bsq = 2 * m * bm + bm * bm + U * (m + bm) ** 2                          # the rounded mean, squared and rounded
    bvar = bq + bsq + U * (q + m * m + bq + bsq)                            # the subtraction
    var = max(q - m * m, 0.0)
    bsd = math.sqrt(bvar) if var <= 0 else min(math.sqrt(bvar), bvar / math.sqrt(var))   # |sqrt a - sqrt b| both ways
    return bm, bsd + U * (math.sqrt(var) + bsd)                             # ... and the root's rounding


def stats_bound(trace):
    """(bound on |mean - model_stats'|, bound on |sd - model_stats'|) for sums made in any order: the device's error with gamma_n
    plus the model's own with one rounding per sum."""
    v = np.asarray(trace, dtype=np.float64).ravel()
    v = v[v != 0]
    n = int(v.size)
    if n == 0:
        return 0.0, 0.0
    gamma = n * U / (1 - n * U)
    sum_abs, q = math.fsum(np.abs(v)), math.fsum(v * v) / n
    mean = math.fsum(v) / n
    dev, own = _propagate(n, sum_abs, q, mean, gamma), _propagate(n, sum_abs, q, mean, U)
    return dev[0] + own[0], dev[1] + own[1]


def model_events(runs, hi, time_of_col, min_gap, min_duration, max_duration, period):
    """event_filter's definition as a plain loop: keep peak > hi, merge within a trace while the gap is < min_gap, then the
    durations.  -> dict like model_runs' (without counts)."""
    kept = [dict(trace=int(t), start=int(a), stop=int(b), peak_col=int(c), peak=np.float32(p))
            for t, a, b, c, p in zip(runs["trace"], runs["start"], runs["stop"], runs["peak_col"], runs["peak"])
            if p > np.float32(hi[int(t)])]
    when = (lambda col: col * period) if time_of_col is None else (lambda col: float(time_of_col[col]))
    merged = []
    for e in kept:
        last = merged[-1] if merged else None
        if last is not None and last["trace"] == e["trace"] and when(e["start"]) - when(last["stop"] - 1) < min_gap:
            last["stop"] = e["stop"]
            if e["peak"] > last["peak"]:
                last["peak"], last["peak_col"] = e["peak"], e["peak_col"]
        else:
            merged.append(dict(e))
    out = [e for e in merged if (e["stop"] - e["start"]) * period >= min_duration
           and (max_duration is None or (e["stop"] - e["start"]) * period <= max_duration)]
    res = {k: np.array([e[k] for e in out], dtype=np.int64) for k in ("trace", "start", "stop", "peak_col")}
    res["peak"] = np.array([e["peak"] for e in out], dtype=np.float32)
    return res


# -- the recording of the end-to-end tests ---------------------------------------------------------------------------------
FS = 1000.0
N = 8192
SPLIT = 4096                                                                # the first sample of the second epoch ...
GAP_SECONDS = 2.0                                                           # ... which begins this much later on the clock
BURST = 60                                                                  # samples: 60 ms of 150 Hz
# first samples of the bursts: one ends 30 ms before the first epoch does; two of channel 1 lie 40 ms apart
BURSTS = {0: (500, 2000, SPLIT - 30 - BURST, 6000), 1: (1200, 3000, 3000 + BURST + 40, 7000)}
BAND = (120.0, 200.0)
TRANSFORM = dict(freq_limits=[100, 250], voices_per_octave=4)


def recording(amplitude=6.0, seed=7):
    """(x (2, N) float32: white noise of sd 1 plus the bursts, timestamps (N,): two epochs with a gap on the clock)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((2, N))
    for ch, firsts in BURSTS.items():
        for a in firsts:
            x[ch, a:a + BURST] += amplitude * np.cos(2 * np.pi * 150.0 * np.arange(BURST) / FS)
    ts = np.arange(N) / FS
    ts[SPLIT:] += GAP_SECONDS
    return x.astype(np.float32), ts


def found(channel, peak_time, start_col, stop_col, timestamps, stride=1, bursts=BURSTS):
    """Why the events are not the bursts, each found exactly once in its channel with the peak inside it and no event reaching
    from one epoch into the other: a list of complaints, empty when all is well."""
    wrong = []
    split = -(-SPLIT // stride)                                             # the first column of the second epoch
    for a, b in zip(start_col, stop_col):
        if a < split < b:
            wrong.append("an event spans the gap: columns %d .. %d" % (a, b))
    for ch, firsts in bursts.items():
        times = np.asarray(peak_time)[np.asarray(channel) == ch]
        if len(times) != len(firsts):
            wrong.append("channel %d: %d events for %d bursts" % (ch, len(times), len(firsts)))
        for a in firsts:
            inside = np.count_nonzero((times >= timestamps[a]) & (times <= timestamps[a + BURST - 1]))
            if inside != 1:
                wrong.append("channel %d: %d peaks inside the burst at sample %d" % (ch, inside, a))
    return wrong
