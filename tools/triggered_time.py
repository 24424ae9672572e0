"""triggered() on a resident complex result of 128 ch x 1e6 samples, 23 scales 200 .. 4.4 Hz (23.6 GB), 1000 events,
300 columns before and 700 after (L = 1001): the kernel between HIP events (warm, median), its read rate on the
algorithmic bytes (events x L x 8 B per row), the whole call with its outputs brought over, beside what the same answer
costs without it: `fetch()`-style reads of each event's window (`DeviceResult.to_host`) and the NumPy reduction.  The two
are alternated in one process.  Prints the markdown table of profiles/triggered.md.

    python tools/triggered_time.py [channels] [rounds] [host_rounds] > table.md
    python tools/triggered_time.py [channels] once     one call and nothing else: for a counter pass, e.g.
        rocprofv3 --pmc FETCH_SIZE -d out -- python tools/triggered_time.py 128 once
"""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

FS, N = 1000.0, 1000000
N_EVENTS, NB, NA = 1000, 300, 700


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


def by_hand(result, cols, nb, na):
    """What the answer costs without triggered(): every event's window to the host, reduced there.  -> (the five arrays,
    seconds spent in the reads)."""
    c, s, _ = result.shape
    n_lags = nb + na + 1
    amp, power = np.zeros((c, s, n_lags)), np.zeros((c, s, n_lags))
    evoked, vector = np.zeros((c, s, n_lags), np.complex128), np.zeros((c, s, n_lags), np.complex128)
    t_read = 0.0
    for e in cols:
        t0 = time.perf_counter()
        seg = result.to_host(np.complex64, None, int(e) - nb, int(e) + na + 1)
        t_read += time.perf_counter() - t0
        a = np.abs(seg)
        amp += a
        power += a * a
        evoked += seg
        vector += seg / np.where(a > 0, a, 1)
    k = float(len(cols))
    return {"amplitude": amp / k, "power": power / k, "evoked": evoked / k, "vector": vector / k,
            "itpc": np.minimum(np.abs(vector) / k, 1.0)}, t_read


def main():
    from ghost_amd import _lib, engine
    from ghost_amd.synthetic import lfp
    ch = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    once = len(sys.argv) > 2 and sys.argv[2] == "once"
    rounds = 1 if once else int(sys.argv[2]) if len(sys.argv) > 2 else 11
    host_rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    freqs = 200.0 / 2 ** (np.arange(23) / 4.0)
    plan = engine.CwtPlan(N, ch, FS, freqs, output="complex")
    result = plan.execute_resident(lfp(ch, N, FS))
    c, s, n = result.shape
    cols = np.ascontiguousarray(np.random.default_rng(1).integers(NB, n - NA, N_EVENTS), dtype=np.int64)
    n_lags = NB + NA + 1
    algo = float(N_EVENTS) * n_lags * 8.0 * c * s
    pitch = (n_lags + 31) & ~31
    plane = c * s * pitch * 4
    buf = engine.DeviceBuffer(7 * plane)

    def call():
        base = buf.ptr.value
        engine.check(_lib.lib.gcwt_triggered(result.buffer.ptr, result.pitch, c, s, n, 0, s, cols.ctypes.data_as(C.POINTER(C.c_int64)),
                                             N_EVENTS, NB, NA, C.c_void_p(base + 4 * plane), C.c_void_p(base + 5 * plane),
                                             C.c_void_p(base), C.c_void_p(base + 2 * plane), C.c_void_p(base + 6 * plane), pitch))

    call()                                                  # warm-up: code object, clocks (the one call of `once`)
    if once:
        return
    ev = Events()
    kernel, whole, hand, reads = [], [], [], []
    worst = 0.0
    for r in range(rounds):                                 # alternated
        kernel.append(ev.ms(call))                          # (the entry's copy of the event list and its launch)
        t0 = time.perf_counter()
        res = engine.triggered(result, cols, NB, NA)
        out = res.to_host()
        res.free()
        whole.append((time.perf_counter() - t0) * 1e3)
        if r < host_rounds:
            t0 = time.perf_counter()
            ref, t_read = by_hand(result, cols, NB, NA)
            hand.append((time.perf_counter() - t0) * 1e3)
            reads.append(t_read * 1e3)
            worst = max(worst, float(np.abs(out["power"] - ref["power"]).max() / ref["power"].max()),
                        float(np.abs(out["vector"] - ref["vector"]).max()))
        print("round %d of %d" % (r + 1, rounds), file=sys.stderr, flush=True)
    med = lambda v: float(np.median(v))
    print("Resident result: %d ch x %d samples x %d scales complex64, %.1f GB; %d events, %d + %d + 1 = %d lags, algorithmic "
          "bytes %.2f GB, outputs %.1f MB; medians of %d alternated rounds (%s).  The two answers differ by at most %.1e "
          "(power relative to its largest, vector absolute).\n"
          % (c, n, s, result.nbytes / 1e9, N_EVENTS, NB, NA, n_lags, algo / 1e9, 7 * c * s * n_lags * 4 / 1e6, rounds,
             engine.device_name(), worst))
    print("| what | ms (median) | min | max | GB/s on algorithmic bytes | by hand / this |")
    print("|---|---|---|---|---|---|")
    t, tw = med(kernel), med(whole)
    if hand:
        th = med(hand)
        ratio = lambda v: "%.0f" % (th / v)
    else:
        ratio = lambda v: "not measured"
    print("| gcwt_triggered: the event list's copy and the kernel (HIP events) | %.2f | %.2f | %.2f | %.0f | %s |"
          % (t, min(kernel), max(kernel), algo / 1e9 / (t * 1e-3), ratio(t)))
    print("| ... with its outputs allocated, computed and on the host (wall) | %.2f | %.2f | %.2f | | %s |"
          % (tw, min(whole), max(whole), ratio(tw)))
    if hand:
        print("| by hand: to_host() of each event's window and the NumPy sums (%d rounds) | %.0f | %.0f | %.0f | %.1f | 1 |"
              % (len(hand), th, min(hand), max(hand), algo / 1e9 / (th * 1e-3)))
        print("| ... of which the reads | %.0f | %.0f | %.0f | %.1f (link) | |"
              % (med(reads), min(reads), max(reads), algo / 1e9 / (med(reads) * 1e-3)))


if __name__ == "__main__":
    main()
