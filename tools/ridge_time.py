"""ridge() on a resident complex result of 128 ch x 1e6 samples x 100 scales 200 .. 2 Hz (the headline shape, 102 GB), one
band of all rows: gcwt_ridge between HIP events (warm, median) with all four outputs, without `frequency` (no gathers, no
arctangent) and with `frequency` alone, beside gcwt_bandpass with `envelope` alone on the same rows -- the yardstick: both
kernels read the same bytes -- alternated in one process, and what `gcwt_debug_bandwidth`'s copy reads in the same run.
Prints the markdown table of profiles/ridge.md.

    python tools/ridge_time.py [channels] [rounds] > table.md
"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from triggered_time import Events

FS, N, S = 1000.0, 1000000, 100


def main():
    from ghost_amd import _lib, engine
    from ghost_amd.synthetic import lfp
    from ghost_amd.wave import Morse
    ch = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 9
    freqs = np.geomspace(200.0, 2.0, S)
    plan = engine.CwtPlan(N, ch, FS, freqs, output="complex")
    result = plan.execute_resident(lfp(ch, N, FS))
    c, s, n = result.shape
    g, _ = engine.band_weights(freqs, Morse(fs=FS))
    e = engine.ridge_weights(freqs, Morse(fs=FS))
    nu = (2 * np.pi * freqs / FS).astype(np.float32)
    rows = np.array([[0, s]], dtype=np.int32)
    seg = np.array([[0, n]], dtype=np.int64)
    f32p, i32p, i64p = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    pitch = (n + 31) & ~31
    plane = c * pitch * 4
    buf = engine.DeviceBuffer(4 * plane)
    at = [C.c_void_p(buf.ptr.value + k * plane) for k in range(4)]

    def ridge(row, amp, off, frq):
        engine.check(_lib.lib.gcwt_ridge(result.buffer.ptr, result.pitch, c, s, n, rows.ctypes.data_as(i32p), 1,
                                         e.ctypes.data_as(f32p), nu.ctypes.data_as(f32p), FS, seg.ctypes.data_as(i64p), 1,
                                         row, amp, off, frq, pitch))

    def envelope():
        engine.check(_lib.lib.gcwt_bandpass(result.buffer.ptr, result.pitch, c, s, n, rows.ctypes.data_as(i32p), 1,
                                            g.ctypes.data_as(f32p), None, None, at[0], None, pitch))

    cases = (("gcwt_ridge: row, amplitude, offset, frequency", lambda: ridge(*at), 16),
             ("gcwt_ridge: row, amplitude, offset", lambda: ridge(at[0], at[1], at[2], None), 12),
             ("gcwt_ridge: frequency", lambda: ridge(None, None, None, at[3]), 4),
             ("gcwt_bandpass: envelope (the yardstick)", envelope, 4))
    for _, fn, _ in cases:                                    # warm-up: code objects, clocks
        fn()
    ev = Events()
    probe = C.c_double(0)
    engine.check(_lib.lib.gcwt_debug_bandwidth(1, 1 << 30, C.byref(probe)))      # GCWT_BW_COPY: read 1 GiB, write 1 GiB
    ms = {what: [] for what, _, _ in cases}
    for r in range(rounds):                                   # alternated
        for what, fn, _ in cases:
            ms[what].append(ev.ms(fn))
        print("round %d of %d" % (r + 1, rounds), file=sys.stderr, flush=True)
    yard = float(np.median(ms[cases[-1][0]]))
    print("Resident result: %d ch x %d samples x %d scales complex64, %.1f GB; one band of all rows; medians of %d alternated "
          "rounds (%s); each interval holds the entry's table copies and its launch.  gcwt_debug_bandwidth's copy (1 GiB read, "
          "1 GiB written) in the same process: %.0f GB/s.\n" % (c, n, s, result.nbytes / 1e9, rounds, engine.device_name(), probe.value))
    print("| what | ms (median) | min | max | GB/s on algorithmic bytes | x the yardstick |")
    print("|---|---|---|---|---|---|")
    for what, _, out_bytes in cases:
        t = float(np.median(ms[what]))
        b = c * n * (8.0 * s + out_bytes)                    # every row read once, the outputs written once
        print("| %s | %.2f | %.2f | %.2f | %.0f | %.2f |" % (what, t, min(ms[what]), max(ms[what]), b / 1e9 / (t * 1e-3), t / yard))


if __name__ == "__main__":
    main()
