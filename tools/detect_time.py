"""detect() on a resident complex result of 128 ch x 1e6 samples x 100 scales 200 .. 2 Hz (the headline shape, 102 GB)
with a ten-row band: the steps of ContinuousWaveletTransform.detect() -- bandpass of the band's envelope, gcwt_trace_stats,
gcwt_trace_runs (its sizing call and its writing call), the runs' way to the host, engine.event_filter -- each between a
host clock and the synchronise the entries end in (warm, median), the bytes that cross PCIe, beside what the same
definition costs without it: bandpass(outputs=('envelope',)) to the host and the NumPy run-length scan there.  The two
are alternated in one process and must agree exactly.  Then the same for the robust thresholds of
detect(stats='median'): bandpass, engine.trace_stats, the three selects of engine.trace_median_mad (gcwt_trace_order),
the runs and the filter, beside the by-hand route: the envelope to the host and np.median twice per channel there; the
medians and MADs must agree exactly.  Prints the markdown tables of profiles/detect.md.

    python tools/detect_time.py [channels] [rounds] [host_rounds] > table.md
    python tools/detect_time.py [channels] once     one detect and nothing else: for a kernel trace, e.g.
        rocprofv3 --kernel-trace --stats -d out -- python tools/detect_time.py 128 once
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

FS, N, S = 1000.0, 1000000, 100
BAND_ROWS = (5, 10)                                          # ten rows from row 5: 158 .. 104 Hz
THRESHOLD, EDGE = 3.0, 0.0
ROBUST_THRESHOLD, ROBUST_EDGE = 12.0, 2.0


def on_device(engine, result, rows, g, h, clock):
    """detect()'s steps (ghost_amd/wave/transforms.py), timed one by one.  -> runs after the filter, thresholds."""
    t0 = time.perf_counter()
    res = engine.bandpass(result, rows, g, h, ("envelope",))
    t1 = time.perf_counter()
    c, n = res.n_channels, res.n_cols
    trace = res.buffer.ptr.value + res._offsets()["envelope"]
    _, mean, sd = engine.trace_stats(trace, res.pitch, c, n)
    t2 = time.perf_counter()
    hi, lo = (mean + THRESHOLD * sd).astype(np.float32), (mean + EDGE * sd).astype(np.float32)
    runs = engine.trace_runs(trace, res.pitch, c, n, lo)
    t3 = time.perf_counter()
    res.free()
    ev = engine.event_filter(runs["trace"], runs["start"], runs["stop"], runs["peak_col"], runs["peak"], hi, None, 0.0, 0.0, None, 1 / FS)
    t4 = time.perf_counter()
    for name, dt in (("bandpass", t1 - t0), ("stats", t2 - t1), ("runs", t3 - t2), ("filter", t4 - t3), ("total", t4 - t0)):
        clock.setdefault(name, []).append(dt * 1e3)
    return ev, hi, lo, int(runs["counts"].sum())


def by_hand(engine, result, rows, g, h, clock):
    """The same definition the only way there is without detect(): the envelope to the host, NumPy there."""
    t0 = time.perf_counter()
    res = engine.bandpass(result, rows, g, h, ("envelope",))
    env = res.to_host()["envelope"][:, 0]
    res.free()
    t1 = time.perf_counter()
    out = {k: [] for k in ("trace", "start", "stop", "peak_col", "peak")}
    his = np.zeros(len(env), np.float32)
    for ch, v in enumerate(env):
        live = v[v != 0].astype(np.float64)
        mean = live.mean() if live.size else 0.0
        sd = np.sqrt(max((live * live).mean() - mean * mean, 0.0)) if live.size else 0.0
        his[ch], lo = np.float32(mean + THRESHOLD * sd), np.float32(mean + EDGE * sd)
        edge = np.diff(np.concatenate(([0], (v > lo).astype(np.int8), [0])))
        start, stop = np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)
        if start.size:
            cols = np.flatnonzero(v > lo)                                    # ascending: run after run
            owner = np.cumsum(edge[:-1] == 1)[cols] - 1
            peak = np.maximum.reduceat(v[cols], np.concatenate(([0], np.cumsum(stop - start)[:-1])))
            hit = np.flatnonzero(v[cols] == peak[owner])                     # the first of them in every run
            first = cols[hit[np.concatenate(([True], owner[hit][1:] != owner[hit][:-1]))]]
        else:
            peak, first = np.zeros(0, np.float32), np.zeros(0, np.int64)
        out["trace"].append(np.full(start.size, ch, np.int64)), out["start"].append(start), out["stop"].append(stop)
        out["peak_col"].append(first), out["peak"].append(peak)
    runs = {k: np.concatenate(v) for k, v in out.items()}
    ev = engine.event_filter(runs["trace"], runs["start"], runs["stop"], runs["peak_col"], runs["peak"], his, None, 0.0, 0.0, None, 1 / FS)
    t2 = time.perf_counter()
    for name, dt in (("hand: envelope to the host", t1 - t0), ("hand: NumPy", t2 - t1), ("hand: total", t2 - t0)):
        clock.setdefault(name, []).append(dt * 1e3)
    return ev, env.nbytes


def robust_on_device(engine, result, rows, g, h, clock):
    """detect(stats='median')'s steps, timed one by one; trace_median_mad's three selects apart.  -> events, median, mad, runs."""
    t0 = time.perf_counter()
    res = engine.bandpass(result, rows, g, h, ("envelope",))
    t1 = time.perf_counter()
    c, n = res.n_channels, res.n_cols
    trace = res.buffer.ptr.value + res._offsets()["envelope"]
    engine.trace_stats(trace, res.pitch, c, n)
    t2 = time.perf_counter()
    split, real = [], engine.trace_order

    def timed(*args):
        a = time.perf_counter()
        out = real(*args)
        split.append(time.perf_counter() - a)
        return out

    engine.trace_order = timed
    try:
        _, median, mad = engine.trace_median_mad(trace, res.pitch, c, n)
    finally:
        engine.trace_order = real
    t3 = time.perf_counter()
    spread = engine.MAD_TO_SD * mad
    hi, lo = (median + ROBUST_THRESHOLD * spread).astype(np.float32), (median + ROBUST_EDGE * spread).astype(np.float32)
    runs = engine.trace_runs(trace, res.pitch, c, n, lo)
    t4 = time.perf_counter()
    res.free()
    ev = engine.event_filter(runs["trace"], runs["start"], runs["stop"], runs["peak_col"], runs["peak"], hi, None, 0.0, 0.0, None, 1 / FS)
    t5 = time.perf_counter()
    for name, dt in (("robust: bandpass", t1 - t0), ("robust: stats", t2 - t1), ("robust: select n", split[0]), ("robust: select median", split[1]),
                     ("robust: select mad", split[2]), ("robust: median_mad", t3 - t2), ("robust: runs", t4 - t3), ("robust: filter", t5 - t4),
                     ("robust: total", t5 - t0)):
        clock.setdefault(name, []).append(dt * 1e3)
    return ev, median, mad, int(runs["counts"].sum())


def robust_by_hand(engine, result, rows, g, h, clock):
    """The thresholds' statistics the only way there is without gcwt_trace_order: the envelope to the host, np.median twice."""
    t0 = time.perf_counter()
    res = engine.bandpass(result, rows, g, h, ("envelope",))
    env = res.to_host()["envelope"][:, 0]
    res.free()
    t1 = time.perf_counter()
    median, mad = np.zeros(len(env)), np.zeros(len(env))
    for ch, v in enumerate(env):
        live = v[v != 0]
        if live.size:
            median[ch] = np.median(live.astype(np.float64))
            mad[ch] = np.median(np.abs(live - np.float32(median[ch])).astype(np.float64))
    t2 = time.perf_counter()
    for name, dt in (("robust by hand: envelope to the host", t1 - t0), ("robust by hand: np.median twice per channel", t2 - t1),
                     ("robust by hand: total", t2 - t0)):
        clock.setdefault(name, []).append(dt * 1e3)
    return median, mad, env.nbytes


def main():
    from ghost_amd import engine
    from ghost_amd.synthetic import lfp
    from ghost_amd.wave import Morse
    ch = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    once = len(sys.argv) > 2 and sys.argv[2] == "once"
    rounds = 1 if once else int(sys.argv[2]) if len(sys.argv) > 2 else 7
    host_rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 2
    freqs = np.geomspace(200.0, 2.0, S)
    plan = engine.CwtPlan(N, ch, FS, freqs, output="complex")
    result = plan.execute_resident(lfp(ch, N, FS))
    g, h = engine.band_weights(freqs, Morse(fs=FS))
    rows = np.array([BAND_ROWS], dtype=np.int32)
    on_device(engine, result, rows, g, h, {})                # warm-up: code objects, clocks (the one call of `once`)
    robust_on_device(engine, result, rows, g, h, {})
    if once:
        return
    clock, agree = {}, True
    for r in range(rounds):                                  # alternated
        ev, hi, lo, n_runs = on_device(engine, result, rows, g, h, clock)
        if r < host_rounds:
            ref, env_bytes = by_hand(engine, result, rows, g, h, clock)
            agree = agree and all(ev[k].tobytes() == ref[k].tobytes() for k in ev)
        print("round %d of %d" % (r + 1, rounds), file=sys.stderr, flush=True)
    c, s, n = result.shape
    first, count = BAND_ROWS
    print("Resident result: %d ch x %d samples x %d scales complex64, %.1f GB; band: rows %d .. %d (%.0f .. %.0f Hz); envelope, "
          "hi = mean + %g sd, lo = mean + %g sd; medians of %d alternated rounds, %d by hand (%s).  %d runs above lo, %d events; "
          "the two event lists are %s.\n"
          % (c, n, s, result.nbytes / 1e9, first, first + count - 1, freqs[first], freqs[first + count - 1], THRESHOLD, EDGE, rounds,
             min(rounds, host_rounds), engine.device_name(), n_runs, len(ev["trace"]), "identical" if agree else "DIFFERENT"))
    print("| what | ms (median) | min | max | bytes over PCIe |")
    print("|---|---|---|---|---|")
    crossing = {"bandpass": 8 * s + 8, "stats": 24 * c, "runs": 2 * (4 * c + 8 * (c + 1)) + 28 * n_runs, "total": 8 * s + 8 + 24 * c
                + 2 * (4 * c + 8 * (c + 1)) + 28 * n_runs, "hand: envelope to the host": env_bytes if host_rounds else 0,
                "hand: total": env_bytes if host_rounds else 0}
    names = {"bandpass": "engine.bandpass: the band's envelope, left on the device", "stats": "engine.trace_stats",
             "runs": "engine.trace_runs: sizing call, writing call, the records to the host", "filter": "engine.event_filter (host)",
             "total": "all of detect()'s steps"}
    for key, v in clock.items():
        print("| %s | %.2f | %.2f | %.2f | %s |" % (names.get(key, key), np.median(v), min(v), max(v), crossing.get(key, "")))

    clock, agree = {}, True
    for r in range(rounds):                                  # alternated
        ev, median, mad, n_runs = robust_on_device(engine, result, rows, g, h, clock)
        if r < host_rounds:
            ref_median, ref_mad, env_bytes = robust_by_hand(engine, result, rows, g, h, clock)
            agree = agree and median.tobytes() == ref_median.tobytes() and mad.tobytes() == ref_mad.tobytes()
        print("robust round %d of %d" % (r + 1, rounds), file=sys.stderr, flush=True)
    print("\nstats='median': hi = median + %g x 1.4826 MAD, lo = median + %g x 1.4826 MAD; %d runs above lo, %d events; medians "
          "%.4g .. %.4g, MADs %.4g .. %.4g; the device's medians and MADs and NumPy's on the host are %s.\n"
          % (ROBUST_THRESHOLD, ROBUST_EDGE, n_runs, len(ev["trace"]), median.min(), median.max(), mad.min(), mad.max(),
             "identical" if agree else "DIFFERENT"))
    print("| what | ms (median) | min | max | bytes over PCIe |")
    print("|---|---|---|---|---|")
    select = 4 * c + 16 * c + 8 * c + 8 * c                  # centres, ranks down; n and two values up
    crossing = {"robust: bandpass": 8 * s + 8, "robust: stats": 24 * c, "robust: select n": select - 4 * c, "robust: select median": select - 4 * c,
                "robust: select mad": select, "robust: median_mad": 3 * select - 8 * c, "robust: runs": 2 * (4 * c + 8 * (c + 1)) + 28 * n_runs,
                "robust: total": 8 * s + 8 + 24 * c + 3 * select - 8 * c + 2 * (4 * c + 8 * (c + 1)) + 28 * n_runs,
                "robust by hand: envelope to the host": env_bytes if host_rounds else 0, "robust by hand: total": env_bytes if host_rounds else 0}
    for key, v in clock.items():
        print("| %s | %.2f | %.2f | %.2f | %s |" % (key, np.median(v), min(v), max(v), crossing.get(key, "")))


if __name__ == "__main__":
    main()
