"""gcwt_trace_smooth and detect(smooth=) on the MI355X.  First the kernel alone on 128 traces of 1e6 columns (512 MB in, 512
MB out), between a host clock and the synchronise the entry ends in (warm, median): at half = 16 (a Gaussian of sd 4 ms at
1 kHz), where it should be bound by memory, beside `gcwt_debug_bandwidth`'s copy of the same bytes on the same machine in
the same run, alternated; and at half = 480 (sd 4 ms at 30 kHz), where the arithmetic decides, as columns per second.  Then
detect()'s steps on a resident complex result of 128 ch x 1e6 samples x 100 scales 200 .. 2 Hz (the headline shape of
tools/detect_time.py, 102 GB) with a ten-row band, with and without smooth=0.004, alternated; the unsmoothed call makes
tools/detect_time.py's launches.  Prints the markdown tables of profiles/smooth.md.

    python tools/smooth_time.py [channels] [rounds] > table.md
    python tools/smooth_time.py [channels] kernel   the first part alone (no transform: seconds, not minutes)
    python tools/smooth_time.py [channels] once     one smoothing at each half and nothing else: for a kernel trace, e.g.
        rocprofv3 --kernel-trace --stats -d out -- python tools/smooth_time.py 128 once
"""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

FS, N, S = 1000.0, 1000000, 100
BAND_ROWS = (5, 10)                                          # ten rows from row 5: 158 .. 104 Hz
THRESHOLD, EDGE = 3.0, 0.0
SMOOTH = 0.004
HALVES = (16, 480)


def gauss(half):
    k = np.arange(half + 1, dtype=np.float64)
    w = np.exp(-0.5 * (k / (half / 4.0)) ** 2)
    return (w / (w[0] + 2 * w[1:].sum())).astype(np.float32)


def kernel_alone(engine, _lib, ch, rounds, once):
    pitch = (N + 31) & ~31
    rng = np.random.default_rng(0)
    src, dst = engine.DeviceBuffer(ch * pitch * 4), engine.DeviceBuffer(ch * pitch * 4)
    for i in range(ch):                                      # a channel at a time: no 512 MB twice on the host
        src.upload(rng.standard_normal(pitch).astype(np.float32), i * pitch * 4)
    f32p = C.POINTER(C.c_float)

    def smooth(w):
        t0 = time.perf_counter()
        engine.check(_lib.lib.gcwt_trace_smooth(src.ptr, pitch, ch, N, w.ctypes.data_as(f32p), len(w) - 1, None, 0, None, 0, dst.ptr, pitch))
        return (time.perf_counter() - t0) * 1e3

    taps = {half: gauss(half) for half in HALVES}
    for half in HALVES:
        smooth(taps[half])                                   # warm-up: code object, clocks (the calls of `once`)
    if once:
        return
    ms, copy = {half: [] for half in HALVES}, []
    for _ in range(rounds):                                  # alternated
        for half in HALVES:
            ms[half].append(smooth(taps[half]))
        gbs = C.c_double(0)
        engine.check(_lib.lib.gcwt_debug_bandwidth(1, ch * N * 4, C.byref(gbs)))   # GCWT_BW_COPY: the same bytes read and written
        copy.append(gbs.value)
    # a spot check that what was timed is the smoother: one column against NumPy
    row = dst.download((pitch,), np.float32, 0)
    v = src.download((pitch,), np.float32, 0).astype(np.float64)
    w = taps[HALVES[-1]].astype(np.float64)
    c = N // 2
    want = w[0] * v[c] + sum(w[k] * (v[c - k] + v[c + k]) for k in range(1, len(w)))
    moved = 2.0 * ch * N * 4
    print("gcwt_trace_smooth alone: %d traces x %d columns float32, %.0f MB read and as much written; host clock around the entry "
          "(it ends in a synchronise), medians of %d alternated rounds (%s).  gcwt_debug_bandwidth's copy of the same bytes in the "
          "same run: %.0f GB/s (median; %.0f .. %.0f).  Column %d of trace 0 at half = %d: %.7g, NumPy in float64: %.7g.\n"
          % (ch, N, moved / 2e6, rounds, engine.device_name(), np.median(copy), min(copy), max(copy), c, HALVES[-1], row[c], want))
    print("| half | ms (median) | min | max | GB/s on the bytes moved | of the copy | columns / s | lane operations / s (2 per tap and column) |")
    print("|---|---|---|---|---|---|---|---|")
    for half in HALVES:
        m = np.median(ms[half])
        rate = moved / m / 1e6
        print("| %d | %.3f | %.3f | %.3f | %.0f | %.2f | %.3g | %.3g |"
              % (half, m, min(ms[half]), max(ms[half]), rate, rate / np.median(copy), ch * N / m * 1e3, 2.0 * half * ch * N / m * 1e3))
    src.free()
    dst.free()


def detect_steps(engine, result, rows, g, h, taps, clock, tag):
    """detect()'s steps (ghost_amd/wave/transforms.py), timed one by one; ``taps``: None, or the smoothing in between."""
    t0 = time.perf_counter()
    res = engine.bandpass(result, rows, g, h, ("envelope",))
    t1 = time.perf_counter()
    c, n, pitch = res.n_channels, res.n_cols, res.pitch
    trace = res.buffer.ptr.value + res._offsets()["envelope"]
    smoothed = None
    if taps is not None:
        smoothed, pitch, _ = engine.trace_smooth(trace, pitch, c, n, taps, engine.segments_of(None, 1 / FS, FS, n))
        res.free()
        trace = smoothed.ptr.value
    t2 = time.perf_counter()
    _, mean, sd = engine.trace_stats(trace, pitch, c, n)
    t3 = time.perf_counter()
    hi, lo = (mean + THRESHOLD * sd).astype(np.float32), (mean + EDGE * sd).astype(np.float32)
    runs = engine.trace_runs(trace, pitch, c, n, lo)
    t4 = time.perf_counter()
    res.free()
    if smoothed is not None:
        smoothed.free()
    ev = engine.event_filter(runs["trace"], runs["start"], runs["stop"], runs["peak_col"], runs["peak"], hi, None, 0.0, 0.0, None, 1 / FS)
    t5 = time.perf_counter()
    for name, dt in (("bandpass", t1 - t0), ("smooth (with its buffer; the band trace freed)", t2 - t1), ("stats", t3 - t2), ("runs", t4 - t3),
                     ("filter", t5 - t4), ("total", t5 - t0)):
        if taps is not None or not name.startswith("smooth"):
            clock.setdefault(tag + name, []).append(dt * 1e3)
    return int(runs["counts"].sum()), len(ev["trace"])


def main():
    from ghost_amd import _lib, engine
    from ghost_amd.synthetic import lfp
    from ghost_amd.wave import Morse
    ch = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    mode = sys.argv[2] if len(sys.argv) > 2 and not sys.argv[2].isdigit() else None
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 and mode is None else 7
    kernel_alone(engine, _lib, ch, rounds, mode == "once")
    if mode is not None:
        return
    freqs = np.geomspace(200.0, 2.0, S)
    plan = engine.CwtPlan(N, ch, FS, freqs, output="complex")
    result = plan.execute_resident(lfp(ch, N, FS))
    g, h = engine.band_weights(freqs, Morse(fs=FS))
    rows = np.array([BAND_ROWS], dtype=np.int32)
    taps = engine.smooth_taps(SMOOTH * FS)
    detect_steps(engine, result, rows, g, h, None, {}, "")   # warm-up
    detect_steps(engine, result, rows, g, h, taps, {}, "")
    clock = {}
    for r in range(rounds):                                  # alternated
        plain = detect_steps(engine, result, rows, g, h, None, clock, "plain: ")
        smooth = detect_steps(engine, result, rows, g, h, taps, clock, "smooth=%g: " % SMOOTH)
        print("round %d of %d" % (r + 1, rounds), file=sys.stderr, flush=True)
    c, s, n = result.shape
    print("\ndetect()'s steps on a resident result of %d ch x %d samples x %d scales complex64, %.1f GB; band: rows %d .. %d; envelope, hi = "
          "mean + %g sd, lo = mean + %g sd; smooth = %g s: sd %g columns, half = %d; medians of %d alternated rounds.  Unsmoothed: %d runs "
          "above lo, %d events; smoothed: %d runs, %d events.\n"
          % (c, n, s, result.nbytes / 1e9, BAND_ROWS[0], sum(BAND_ROWS) - 1, THRESHOLD, EDGE, SMOOTH, SMOOTH * FS, len(taps) - 1, rounds,
             plain[0], plain[1], smooth[0], smooth[1]))
    print("| what | ms (median) | min | max |")
    print("|---|---|---|---|")
    for key, v in clock.items():
        print("| %s | %.2f | %.2f | %.2f |" % (key, np.median(v), min(v), max(v)))


if __name__ == "__main__":
    main()
