"""squeeze() on a resident complex result of 32 ch x 1e6 samples x 100 scales 200 .. 2 Hz (25.6 GB), all rows: gcwt_squeeze
between HIP events (warm, median) with L = 100 and L = 400 cells, `coefficients` alone and all four outputs, and `frequency`
with `index` alone (one walk, nothing summed), beside gcwt_ridge (all four outputs, one band of all rows) and gcwt_bandpass
(`analytic`, one band of all rows: the same sums into one cell) over the same rows, alternated in one process, and what
`gcwt_debug_bandwidth`'s copy reads in the same run.  Prints the markdown table of profiles/squeeze.md.

    python tools/squeeze_time.py [channels] [rounds] > table.md
"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from triggered_time import Events

FS, N, S = 1000.0, 1000000, 100
CELLS = (100, 400)


def main():
    from ghost_amd import _lib, engine
    from ghost_amd.synthetic import lfp
    from ghost_amd.wave import Morse
    ch = int(sys.argv[1]) if len(sys.argv) > 1 else 32
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    freqs = np.geomspace(200.0, 2.0, S)
    plan = engine.CwtPlan(N, ch, FS, freqs, output="complex")
    result = plan.execute_resident(lfp(ch, N, FS))
    c, s, n = result.shape
    g, _ = engine.band_weights(freqs, Morse(fs=FS))
    e = engine.ridge_weights(freqs, Morse(fs=FS))
    nu = (2 * np.pi * freqs / FS).astype(np.float32)
    floor2 = np.zeros(s, np.float32)
    band = np.array([[0, s]], dtype=np.int32)
    seg = np.array([[0, n]], dtype=np.int64)
    edges = {n_cells: engine.squeeze_edges(np.geomspace(freqs[0], freqs[-1], n_cells)) for n_cells in CELLS}
    f32p, i32p, i64p = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    pitch = (n + 31) & ~31
    plane = c * pitch * 4                                      # one float32 row per channel
    most = max(CELLS)
    buf = engine.DeviceBuffer(plane * (3 * most + 2 * s))     # coefficients, power: most rows; frequency, index: s rows
    at = {"coefficients": C.c_void_p(buf.ptr.value), "power": C.c_void_p(buf.ptr.value + 2 * most * plane),
          "frequency": C.c_void_p(buf.ptr.value + 3 * most * plane), "index": C.c_void_p(buf.ptr.value + (3 * most + s) * plane)}
    small = [C.c_void_p(buf.ptr.value + k * plane) for k in range(4)]

    def squeeze(n_cells, names):
        ed, desc = edges[n_cells]
        engine.check(_lib.lib.gcwt_squeeze(result.buffer.ptr, result.pitch, c, s, n, 0, s, g.ctypes.data_as(f32p),
                                           floor2.ctypes.data_as(f32p), nu.ctypes.data_as(f32p), FS, seg.ctypes.data_as(i64p), 1,
                                           ed.ctypes.data_as(f32p), n_cells, int(desc), *[at[k] if k in names else None for k in
                                                                                           ("coefficients", "power", "frequency", "index")],
                                           pitch))

    def ridge():
        engine.check(_lib.lib.gcwt_ridge(result.buffer.ptr, result.pitch, c, s, n, band.ctypes.data_as(i32p), 1,
                                         e.ctypes.data_as(f32p), nu.ctypes.data_as(f32p), FS, seg.ctypes.data_as(i64p), 1,
                                         *small, pitch))

    def analytic():
        engine.check(_lib.lib.gcwt_bandpass(result.buffer.ptr, result.pitch, c, s, n, band.ctypes.data_as(i32p), 1,
                                            g.ctypes.data_as(f32p), None, small[0], None, None, pitch))

    every = ("coefficients", "power", "frequency", "index")
    cases = [("gcwt_squeeze: frequency, index (L = 100, one walk)", lambda: squeeze(100, ("frequency", "index")), 8.0 * s, 1)]
    for n_cells in CELLS:
        walks = -(-n_cells // _lib.SQUEEZE_GROUP_CELLS)
        cases.append(("gcwt_squeeze: coefficients, L = %d (%d walks)" % (n_cells, walks),
                      lambda k=n_cells: squeeze(k, ("coefficients",)), 8.0 * n_cells, walks))
        cases.append(("gcwt_squeeze: all four outputs, L = %d (%d walks)" % (n_cells, walks),
                      lambda k=n_cells: squeeze(k, every), 12.0 * n_cells + 8.0 * s, walks))
    cases.append(("gcwt_ridge: row, amplitude, offset, frequency", ridge, 16.0, 1))
    cases.append(("gcwt_bandpass: analytic", analytic, 8.0, 1))
    for _, fn, _, _ in cases:                                 # warm-up: code objects, clocks
        fn()
    ev = Events()
    probe = C.c_double(0)
    engine.check(_lib.lib.gcwt_debug_bandwidth(1, 1 << 30, C.byref(probe)))      # GCWT_BW_COPY: read 1 GiB, write 1 GiB
    ms = {what: [] for what, _, _, _ in cases}
    for r in range(rounds):                                   # alternated
        for what, fn, _, _ in cases:
            ms[what].append(ev.ms(fn))
        print("round %d of %d" % (r + 1, rounds), file=sys.stderr, flush=True)
    print("Resident result: %d ch x %d samples x %d scales complex64, %.1f GB; all rows, floor2 = 0; medians of %d alternated "
          "rounds (%s); each interval holds the entry's table copies and its launch.  gcwt_debug_bandwidth's copy (1 GiB read, "
          "1 GiB written) in the same process: %.0f GB/s.\n" % (c, n, s, result.nbytes / 1e9, rounds, engine.device_name(), probe.value))
    print("| what | ms (median) | min | max | GB/s, rows read once | GB/s, rows read once per walk |")
    print("|---|---|---|---|---|---|")
    for what, _, out_bytes, walks in cases:
        t = float(np.median(ms[what]))
        once = c * n * (8.0 * s + out_bytes)                 # every row read once, the outputs written once
        each = c * n * (8.0 * s * walks + out_bytes)         # what the walks ask of the caches and the memory together
        print("| %s | %.2f | %.2f | %.2f | %.0f | %.0f |" % (what, t, min(ms[what]), max(ms[what]), once / 1e9 / (t * 1e-3),
                                                           each / 1e9 / (t * 1e-3)))


if __name__ == "__main__":
    main()
