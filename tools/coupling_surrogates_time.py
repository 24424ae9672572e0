"""coupling_surrogates() on a resident complex result of 128 ch x 1e6 samples, 23 scales 200 .. 4.4 Hz (23.6 GB), 8 phase
rows (4 .. 16 Hz) x 11 amplitude rows (30 .. 200 Hz), windows 2048 and 1000, K = 200 shifts: the call between HIP events
(warm, median) and the whole call with its outputs on the host, beside gcwt_coupling at the same shape -- K times that
is what K passes over the rows would cost -- and the arithmetic floor, 2 K C N P A fused multiply-adds.  Prints the
markdown table of profiles/coupling_surrogates.md.

    python tools/coupling_surrogates_time.py [channels] [rounds] [K] > table.md
"""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from coupling_time import Events

FS, N = 1000.0, 1000000
WINDOWS = (2048, 1000)
PEAK_FMA = 157.3e12 / 2                                    # float32 vector peak of an MI355X, fused multiply-adds / s


def main():
    from ghost_amd import _lib, engine
    from ghost_amd.synthetic import lfp
    ch = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 11
    k = int(sys.argv[3]) if len(sys.argv) > 3 else 200
    freqs = 200.0 / 2 ** (np.arange(23) / 4.0)
    ph, am = engine.coupling_rows((4, 16), freqs, "phase"), engine.coupling_rows((30, 200), freqs, "amplitude")
    assert (ph[1], am[1]) == (8, 11)
    plan = engine.CwtPlan(N, ch, FS, freqs, output="complex")
    result = plan.execute_resident(lfp(ch, N, FS))
    c, s, n = result.shape
    shifts = {w: engine.surrogate_shifts(k, w, 227, 0) for w in WINDOWS}

    def surrogates(window, buf, pitch):
        plane = c * ph[1] * am[1] * pitch * 4
        base = buf.ptr.value
        sh = shifts[window]
        engine.check(_lib.lib.gcwt_coupling_surrogates(result.buffer.ptr, result.pitch, c, s, n, ph[0], ph[1], am[0], am[1],
                                                       window, sh.ctypes.data_as(C.POINTER(C.c_int64)), sh.size,
                                                       C.c_void_p(base), C.c_void_p(base + plane), C.c_void_p(base + 2 * plane),
                                                       None, pitch))

    def coupling(window, buf, pitch):
        rows = c * ph[1] * am[1] * pitch
        base = buf.ptr.value
        engine.check(_lib.lib.gcwt_coupling(result.buffer.ptr, result.pitch, c, s, n, ph[0], ph[1], am[0], am[1], window,
                                            C.c_void_p(base), C.c_void_p(base + rows * 8), C.c_void_p(base + rows * 12), pitch))

    bufs = {}
    for w in WINDOWS:
        pitch = (-(-n // w) + 31) & ~31
        bufs[w] = (engine.DeviceBuffer((3 * ph[1] + 1) * c * am[1] * pitch * 4), pitch)
        surrogates(w, *bufs[w])                             # warm-up: code object, clocks
        coupling(w, *bufs[w])
    ev = Events()
    t_sur = {w: [] for w in WINDOWS}
    t_cpl = {w: [] for w in WINDOWS}
    whole = {w: [] for w in WINDOWS}
    for _ in range(rounds):                                 # alternated
        for w in WINDOWS:
            t_sur[w].append(ev.ms(lambda: surrogates(w, *bufs[w])))
            t_cpl[w].append(ev.ms(lambda: coupling(w, *bufs[w])))
            t0 = time.perf_counter()
            res = engine.coupling_surrogates(result, ph, am, w, shifts[w])
            res.to_host()
            res.free()
            whole[w].append((time.perf_counter() - t0) * 1e3)
    med = lambda v: float(np.median(v))
    fma = 2.0 * k * c * n * ph[1] * am[1]
    print("Resident result: %d ch x %d samples x %d scales complex64, %.1f GB; %d phase x %d amplitude rows, K = %d shifts: "
          "%.3g fused multiply-adds, %.1f ms at the vector peak; medians of %d alternated rounds (%s).\n"
          % (c, n, s, result.nbytes / 1e9, ph[1], am[1], k, fma, fma / PEAK_FMA * 1e3, rounds, engine.device_name()))
    print("| what | ms (median) | min | max | of the arithmetic floor | K x gcwt_coupling / this |")
    print("|---|---|---|---|---|---|")
    for w in WINDOWS:
        t, tc = med(t_sur[w]), med(t_cpl[w])
        print("| gcwt_coupling_surrogates, window %d (HIP events) | %.2f | %.2f | %.2f | %.2f x | %.1f |"
              % (w, t, min(t_sur[w]), max(t_sur[w]), t / (fma / PEAK_FMA * 1e3), k * tc / t))
        tw = med(whole[w])
        print("| ... with its outputs allocated, computed and on the host (wall) | %.2f | %.2f | %.2f | | %.1f |"
              % (tw, min(whole[w]), max(whole[w]), k * tc / tw))
        print("| gcwt_coupling, window %d (HIP events) | %.2f | %.2f | %.2f | | %d x this = %.0f ms |"
              % (w, tc, min(t_cpl[w]), max(t_cpl[w]), k, k * tc))


if __name__ == "__main__":
    main()
