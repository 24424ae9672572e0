"""coherence() on a resident complex result of 32 ch x 1e6 samples x 100 scales (25.6 GB), window 1000: seed mode (31
pairs) and all 496 pairs, beside what the same result costs on its way to the host (`to_host(np.complex64)`) and a plain
device copy of it (the read-once floor: `gcwt_debug_bandwidth(GCWT_BW_COPY)`), alternated in one process, medians.
Prints the markdown table of profiles/coherence.md.

    python tools/coherence_time.py [channels] [rounds] > table.md
"""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from ghost_amd import _lib, engine
from ghost_amd.synthetic import lfp

FS, N, S, WINDOW = 1000.0, 1000000, 100, 1000
CH = int(sys.argv[1]) if len(sys.argv) > 1 else 32
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
PEAK_FP32 = 157.3e12                       # vector FP32 flops of the chip (256 CUs x 128 lanes x 2 x 2.4 GHz)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def kernel_call(result, pairs, buf, pitch):
    """gcwt_coherence alone on outputs that exist: tables, launch, synchronise."""
    c, s, n = result.shape
    p = len(pairs)
    base = buf.ptr.value
    rows = p * s * pitch
    engine.check(_lib.lib.gcwt_coherence(result.buffer.ptr, result.pitch, c, s, n, pairs.ctypes.data_as(C.POINTER(C.c_int32)), p,
                                         WINDOW, C.c_void_p(base + rows * 12), C.c_void_p(base), C.c_void_p(base + rows * 8), pitch))


def rows_read(pairs):
    """Rows of one scale the tasks of a pair list read (include/ghostcwt_debug.h: gcwt_debug_coherence_tasks): per task
    the channels its cells name, and every channel of a tile whose power it writes."""
    i32p = C.POINTER(C.c_int32)
    pp = pairs.ctypes.data_as(i32p)
    n = _lib.lib.gcwt_debug_coherence_tasks(CH, pp, len(pairs), None, None, None, None, None, 0)
    ta, tb, fl, first = (np.zeros(n + 1, np.int32) for _ in range(4))
    ent = np.zeros((len(pairs), 3), np.int32)
    _lib.lib.gcwt_debug_coherence_tasks(CH, pp, len(pairs), ta.ctypes.data_as(i32p), tb.ctypes.data_as(i32p),
                                        fl.ctypes.data_as(i32p), first.ctypes.data_as(i32p), ent.ctypes.data_as(i32p), n)
    total = 0
    for t in range(n):
        cells = ent[first[t]:first[t + 1], 0]
        a, b = set((cells // 8).tolist()), set((cells % 8).tolist())
        if fl[t] & 1:
            a |= set(range(min(8, CH - 8 * ta[t])))
        if fl[t] & 2:
            b |= set(range(min(8, CH - 8 * tb[t])))
        total += len(a | b) if ta[t] == tb[t] else len(a) + len(b)
    return total


def main():
    freqs = np.geomspace(300.0, 1.0, S)
    plan = engine.CwtPlan(N, CH, FS, freqs, output="complex")
    result = plan.execute_resident(lfp(CH, N, FS))
    n_bins = -(-N // WINDOW)
    pitch = (n_bins + 31) & ~31
    modes = {"seed (channel 0, %d pairs)" % (CH - 1): engine.coherence_pairs(None, 0, CH),
             "all pairs (%d)" % (CH * (CH - 1) // 2): engine.coherence_pairs(None, None, CH)}
    bufs = {k: engine.DeviceBuffer((3 * len(p) + CH) * S * pitch * 4) for k, p in modes.items()}
    times = {k: [] for k in modes}
    whole = {k: [] for k in modes}
    host, copy = [], []
    for k, p in modes.items():                              # warm-up: code objects, clocks
        kernel_call(result, p, bufs[k], pitch)
    for _ in range(ROUNDS):                                 # alternated: A B H C  A B H C ...
        for k, p in modes.items():
            times[k].append(timed(lambda: kernel_call(result, p, bufs[k], pitch))[0])

            def call_and_fetch():
                r = engine.coherence(result, p, WINDOW)
                out = r.to_host()
                r.free()
                return out
            whole[k].append(timed(call_and_fetch)[0])
        ms, w = timed(lambda: result.to_host(np.complex64))
        host.append(ms)
        del w
        gbs = C.c_double(0)
        engine.check(_lib.lib.gcwt_debug_bandwidth(1, result.nbytes, C.byref(gbs)))
        copy.append(2.0 * result.nbytes / (gbs.value * 1e9) * 1e3)
    med = lambda v: float(np.median(v))
    t_host = med(host)
    print("Resident result: %d ch x %d samples x %d scales complex64, %.1f GB; window %d (%d bins); medians of %d "
          "alternated rounds, one box (%s).\n" % (CH, N, S, result.nbytes / 1e9, WINDOW, n_bins, ROUNDS, engine.device_name()))
    print("| what | ms (median) | min | max | rows read / rows of the result | GB/s of rows read | of FP32 vector peak | "
          "to_host / this |")
    print("|---|---|---|---|---|---|---|---|")
    for k, p in modes.items():
        rows = rows_read(p)
        t = med(times[k])
        flops = 8.0 * len(p) * S * N
        print("| gcwt_coherence, %s | %.2f | %.2f | %.2f | %.2f | %.0f | %.3f | %.1f |"
              % (k, t, min(times[k]), max(times[k]), rows / CH, rows / CH * result.nbytes / 1e9 / (t * 1e-3),
                 flops / (t * 1e-3) / PEAK_FP32, t_host / t))
        tw = med(whole[k])
        print("| ... with its outputs allocated, computed and on the host (%.0f MB) | %.2f | %.2f | %.2f | | | | %.1f |"
              % ((3 * len(p) + CH) * S * n_bins * 4 / 1e6, tw, min(whole[k]), max(whole[k]), t_host / tw))
    print("| to_host(np.complex64) of the result | %.0f | %.0f | %.0f | | %.1f (link) | | 1.0 |"
          % (t_host, min(host), max(host), result.nbytes / 1e9 / (t_host * 1e-3)))
    tc = med(copy)
    print("| device copy of the result (read + write; reading once is half) | %.2f | %.2f | %.2f | 1.00 | %.0f | | %.1f |"
          % (tc, min(copy), max(copy), 2 * result.nbytes / 1e9 / (tc * 1e-3), t_host / tc))


if __name__ == "__main__":
    main()
