"""coupling() on a resident complex result of 128 ch x 1e6 samples, 23 scales 200 .. 4.4 Hz (23.6 GB), 8 phase rows
(4 .. 16 Hz) x 11 amplitude rows (30 .. 200 Hz), windows 1000 and 10000: the kernel between HIP events (warm, median),
its read rate on the algorithmic bytes (19 rows x channels x samples x 8 B), beside what the same answer cost before:
`to_host()` of the 19 rows, the time before NumPy starts.  Prints the markdown table of profiles/coupling.md.

    python tools/coupling_time.py [channels] [rounds] > table.md
    python tools/coupling_time.py [channels] once     one call per window and nothing else: for a counter pass, e.g.
        rocprofv3 --pmc FETCH_SIZE -d out -- python tools/coupling_time.py 128 once
    python tools/coupling_time.py fetch_size <counter_collection.csv>      FETCH_SIZE of k_coupling from that pass
"""
import csv
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

FS, N = 1000.0, 1000000
WINDOWS = (1000, 10000)


def fetch_size(path):
    """Per dispatch of k_coupling, in order: FETCH_SIZE (KiB read through the L2 from memory, as rocprofv3 counts it)."""
    out = []
    for row in csv.DictReader(open(path)):
        if "k_coupling" in row.get("Kernel_Name", "") and row.get("Counter_Name") == "FETCH_SIZE":
            out.append((int(row["Dispatch_Id"]), float(row["Counter_Value"])))
    by = {}
    for d, v in out:                                        # (one row per XCD or one per dispatch: summed either way)
        by[d] = by.get(d, 0.0) + v
    return [by[d] for d in sorted(by)]


class Events:
    """Two HIP events on the null stream, where the library launches."""

    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so")
        self.a, self.b = C.c_void_p(), C.c_void_p()
        assert self.hip.hipEventCreate(C.byref(self.a)) == 0 and self.hip.hipEventCreate(C.byref(self.b)) == 0

    def ms(self, fn):
        assert self.hip.hipEventRecord(self.a, None) == 0
        fn()
        assert self.hip.hipEventRecord(self.b, None) == 0
        assert self.hip.hipEventSynchronize(self.b) == 0
        t = C.c_float(0)
        assert self.hip.hipEventElapsedTime(C.byref(t), self.a, self.b) == 0
        return t.value


def main():
    from ghost_amd import _lib, engine
    from ghost_amd.synthetic import lfp
    ch = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    once = len(sys.argv) > 2 and sys.argv[2] == "once"
    rounds = 1 if once else int(sys.argv[2]) if len(sys.argv) > 2 else 11
    freqs = 200.0 / 2 ** (np.arange(23) / 4.0)
    ph, am = engine.coupling_rows((4, 16), freqs, "phase"), engine.coupling_rows((30, 200), freqs, "amplitude")
    assert (ph[1], am[1]) == (8, 11)
    plan = engine.CwtPlan(N, ch, FS, freqs, output="complex")
    result = plan.execute_resident(lfp(ch, N, FS))
    c, s, n = result.shape
    algo = (ph[1] + am[1]) * c * n * 8.0

    def call(window, buf, pitch):
        rows = c * ph[1] * am[1] * pitch
        base = buf.ptr.value
        engine.check(_lib.lib.gcwt_coupling(result.buffer.ptr, result.pitch, c, s, n, ph[0], ph[1], am[0], am[1], window,
                                            C.c_void_p(base), C.c_void_p(base + rows * 8), C.c_void_p(base + rows * 12), pitch))

    bufs = {}
    for w in WINDOWS:
        pitch = (-(-n // w) + 31) & ~31
        bufs[w] = (engine.DeviceBuffer((3 * ph[1] + 1) * c * am[1] * pitch * 4), pitch)
        call(w, *bufs[w])                                   # warm-up: code object, clocks (the one call of `once`)
    if once:
        return
    ev = Events()
    times = {w: [] for w in WINDOWS}
    whole = {w: [] for w in WINDOWS}
    host = []
    for r in range(rounds):                                 # alternated
        for w in WINDOWS:
            times[w].append(ev.ms(lambda: call(w, *bufs[w])))
            t0 = time.perf_counter()
            res = engine.coupling(result, ph, am, w)
            res.to_host()
            res.free()
            whole[w].append((time.perf_counter() - t0) * 1e3)
        if r < 3:                                           # what the parent offers: the 19 rows to the host
            t0 = time.perf_counter()
            a = result.to_host(np.complex64, scales=slice(ph[0], ph[0] + ph[1]))
            b = result.to_host(np.complex64, scales=slice(am[0], am[0] + am[1]))
            host.append((time.perf_counter() - t0) * 1e3)
            del a, b
    med = lambda v: float(np.median(v))
    print("Resident result: %d ch x %d samples x %d scales complex64, %.1f GB; %d phase x %d amplitude rows, algorithmic "
          "bytes %.2f GB; medians of %d alternated rounds (%s).\n" % (c, n, s, result.nbytes / 1e9, ph[1], am[1], algo / 1e9,
                                                                      rounds, engine.device_name()))
    print("| what | ms (median) | min | max | GB/s on algorithmic bytes | to_host of the 19 rows / this |")
    print("|---|---|---|---|---|---|")
    t_host = med(host)
    for w in WINDOWS:
        t = med(times[w])
        print("| gcwt_coupling, window %d (HIP events) | %.2f | %.2f | %.2f | %.0f | %.0f |"
              % (w, t, min(times[w]), max(times[w]), algo / 1e9 / (t * 1e-3), t_host / t))
        tw = med(whole[w])
        print("| ... with its outputs allocated, computed and on the host (wall) | %.2f | %.2f | %.2f | | %.0f |"
              % (tw, min(whole[w]), max(whole[w]), t_host / tw))
    print("| to_host(np.complex64) of the 8 + 11 rows (%d rounds) | %.0f | %.0f | %.0f | %.1f (link) | 1 |"
          % (len(host), t_host, min(host), max(host), algo / 1e9 / (t_host * 1e-3)))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "fetch_size":
        sizes = fetch_size(sys.argv[2])
        algo = 19 * 128 * N * 8.0
        for w, kib in zip(WINDOWS, sizes):
            print("window %d: FETCH_SIZE %.0f KiB = %.2f GB = %.2f x the algorithmic bytes (128 channels)"
                  % (w, kib, kib * 1024 / 1e9, kib * 1024 / algo))
    else:
        main()
