"""bandpass() on a resident complex result of 128 ch x 1e6 samples, 23 scales 200 .. 4.4 Hz (23.6 GB), two bands: the
entry between HIP events (warm, median), its rate on the algorithmic bytes (the union of the bands' rows read once plus
the outputs written once), beside what `gcwt_debug_bandwidth`'s copy reads on the same machine in the same run, and what
the same answer costs by hand: `to_host()` of the bands' rows and the NumPy sums -- on the first 16 channels, where the
rows still fit a host buffer, against the entry on the same 16.  Prints the markdown table of profiles/bandpass.md.

    python tools/bandpass_time.py [channels] [rounds] [host_rounds] > table.md
    python tools/bandpass_time.py [channels] once     one call and nothing else: for a counter pass, e.g.
        rocprofv3 --pmc FETCH_SIZE -d out -- python tools/bandpass_time.py 128 once
"""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from triggered_time import Events

FS, N = 1000.0, 1000000
CASES = (("theta 4 .. 12 Hz and ripple 80 .. 200 Hz", [(4.0, 12.0), (80.0, 200.0)]),
         ("all rows and theta", [(4.0, 200.0), (4.0, 12.0)]))
HAND_CHANNELS = 16


def by_hand(result, rows, g, h):
    """What the answer costs without bandpass(): the rows of every band to the host, summed there.  -> (analytic,
    envelope, power, seconds spent in the reads)."""
    c, _, n = result.shape
    z, p = np.zeros((c, len(rows), n), np.complex64), np.zeros((c, len(rows), n), np.float32)
    t_read = 0.0
    for k, (a, m) in enumerate(rows):
        t0 = time.perf_counter()
        w = result.to_host(np.complex64, slice(int(a), int(a + m)))
        t_read += time.perf_counter() - t0
        z[:, k] = np.tensordot(g[a:a + m], w, axes=(0, 1))
        p[:, k] = np.tensordot(h[a:a + m], w.real ** 2 + w.imag ** 2, axes=(0, 1))
    return z, np.abs(z), p, t_read


def main():
    from ghost_amd import _lib, engine
    from ghost_amd.synthetic import lfp
    from ghost_amd.wave import Morse
    ch = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    once = len(sys.argv) > 2 and sys.argv[2] == "once"
    rounds = 1 if once else int(sys.argv[2]) if len(sys.argv) > 2 else 11
    host_rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 2
    freqs = 200.0 / 2 ** (np.arange(23) / 4.0)
    plan = engine.CwtPlan(N, ch, FS, freqs, output="complex")
    result = plan.execute_resident(lfp(ch, N, FS))
    c, s, n = result.shape
    g, h = engine.band_weights(freqs, Morse(fs=FS))
    f32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    pitch = (n + 31) & ~31
    n_bands = 2
    plane = c * n_bands * pitch * 4
    buf = engine.DeviceBuffer(4 * plane)                    # analytic (two planes' worth), envelope, power

    def entry(res, rows):
        base = buf.ptr.value
        cc = res.shape[0]
        engine.check(_lib.lib.gcwt_bandpass(res.buffer.ptr, res.pitch, cc, s, n, rows.ctypes.data_as(i32p), len(rows),
                                            g.ctypes.data_as(f32p), h.ctypes.data_as(f32p), C.c_void_p(base),
                                            C.c_void_p(base + 2 * plane), C.c_void_p(base + 3 * plane), pitch))

    tables = [(what, engine.band_rows(bands, freqs)) for what, bands in CASES]
    entry(result, tables[0][1])                             # warm-up: code object, clocks (the one call of `once`)
    if once:
        return
    ev = Events()
    few = engine.DeviceResult(result.buffer, (min(HAND_CHANNELS, c), s, n), result.pitch, True)
    probe = C.c_double(0)
    engine.check(_lib.lib.gcwt_debug_bandwidth(1, 1 << 30, C.byref(probe)))      # GCWT_BW_COPY: read 1 GiB, write 1 GiB
    kernel = {what: [] for what, _ in tables}
    kernel_few, whole, hand, reads = [], [], [], []
    worst = 0.0
    for r in range(rounds):                                 # alternated
        for what, rows in tables:
            kernel[what].append(ev.ms(lambda: entry(result, rows)))              # (the entry's copies and its launch)
        rows = tables[0][1]
        kernel_few.append(ev.ms(lambda: entry(few, rows)))
        t0 = time.perf_counter()
        res = engine.bandpass(few, rows, g, h)
        out = res.to_host()
        res.free()
        whole.append((time.perf_counter() - t0) * 1e3)
        if r < host_rounds:
            t0 = time.perf_counter()
            z, env, p, t_read = by_hand(few, rows, g, h)
            hand.append((time.perf_counter() - t0) * 1e3)
            reads.append(t_read * 1e3)
            worst = max(worst, float(np.abs(out["analytic"] - z).max() / np.abs(z).max()),
                        float(np.abs(out["power"] - p).max() / p.max()))
        print("round %d of %d" % (r + 1, rounds), file=sys.stderr, flush=True)
    med = lambda v: float(np.median(v))

    def algo(cc, rows):
        """Bytes: every row that some band holds read once, 16 bytes written per (channel, band, column)."""
        held = np.zeros(s, bool)
        for a, m in rows:
            held[a:a + m] = True
        return cc * n * (8.0 * np.count_nonzero(held) + 16.0 * len(rows))

    print("Resident result: %d ch x %d samples x %d scales complex64, %.1f GB; two bands, all three outputs (%.1f GB); "
          "medians of %d alternated rounds (%s).  gcwt_debug_bandwidth's copy (1 GiB read, 1 GiB written) in the same "
          "process: %.0f GB/s.  By hand on the first %d channels; the two answers differ by at most %.1e (analytic and "
          "power, each relative to its largest).\n"
          % (c, n, s, result.nbytes / 1e9, c * n_bands * n * 16 / 1e9, rounds, engine.device_name(), probe.value, few.shape[0],
             worst))
    print("| what | ms (median) | min | max | GB/s on algorithmic bytes | share of the probe's rate | by hand / this |")
    print("|---|---|---|---|---|---|---|")
    for what, rows in tables:
        t, b = med(kernel[what]), algo(c, rows)
        print("| gcwt_bandpass, %d ch, %s (rows %s; %.2f GB): copies and kernel (HIP events) | %.2f | %.2f | %.2f | %.0f | %.2f | |"
              % (c, what, " and ".join("%d .. %d" % (a, a + m - 1) for a, m in rows), b / 1e9, t, min(kernel[what]),
                 max(kernel[what]), b / 1e9 / (t * 1e-3), b / 1e9 / (t * 1e-3) / probe.value))
    rows = tables[0][1]
    t, b = med(kernel_few), algo(few.shape[0], rows)
    th = med(hand) if hand else None
    ratio = (lambda v: "%.0f" % (th / v)) if hand else (lambda v: "not measured")
    print("| gcwt_bandpass, %d ch, %s (%.2f GB) | %.2f | %.2f | %.2f | %.0f | %.2f | %s |"
          % (few.shape[0], tables[0][0], b / 1e9, t, min(kernel_few), max(kernel_few), b / 1e9 / (t * 1e-3),
             b / 1e9 / (t * 1e-3) / probe.value, ratio(t)))
    tw = med(whole)
    print("| ... with its outputs allocated, computed and on the host (wall) | %.1f | %.1f | %.1f | | | %s |"
          % (tw, min(whole), max(whole), ratio(tw)))
    if hand:
        print("| by hand, %d ch: to_host() of the bands' rows and the NumPy sums (%d rounds) | %.0f | %.0f | %.0f | %.1f | | 1 |"
              % (few.shape[0], len(hand), th, min(hand), max(hand), b / 1e9 / (th * 1e-3)))
        print("| ... of which the reads | %.0f | %.0f | %.0f | | | |" % (med(reads), min(reads), max(reads)))


if __name__ == "__main__":
    main()
