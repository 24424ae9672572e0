"""Morlet against Morse at the headline shape (128 ch x 1e6 samples at 1 kHz, each wavelet's own default grid,
device-resident): ms per step and per scale, amplitude and complex, runs alternated between the four plans; then per
decimation level (a plan of that level's scales only: ms of its synthesis launches and per scale), with each plan's
method / decimation histogram.  Prints the markdown of profiles/morlet.md.

    python tools/morlet_time.py [channels] > profile.md
"""
import collections
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from ghost_amd.engine import CwtPlan, DeviceBuffer
from ghost_amd.synthetic import lfp
from ghost_amd.wave import Morlet, Morse

FS, N = 1000.0, 1000000
C = int(sys.argv[1]) if len(sys.argv) > 1 else 128
W0 = 6.0
METHODS = {0: "spectral", 1: "direct", 2: "full band", 3: "block conv."}


def default_grid(wavelet):
    lo, hi = np.array(wavelet.compute_freq_bounds(N)) / np.pi * FS / 2.0
    j = np.arange(np.floor(np.log2(hi / lo) * 10) + 1)
    return hi / 2 ** (j / 10.0)


def make(family, output, freqs):
    kw = dict(morlet_w0=W0) if family == "Morlet" else {}
    return CwtPlan(N, C, FS, freqs, output=output, **kw)


def step_ms(plan, xb, ob, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        plan.execute_device(xb, ob)                   # returns when the device is done
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def main():
    grids = {"Morse": default_grid(Morse()), "Morlet": default_grid(Morlet(w0=W0))}
    x = np.tile(lfp(4, N), (C // 4 + 1, 1))[:C]
    xb = DeviceBuffer(x.nbytes)
    xb.upload(x)
    configs = [(fam, out) for out in ("amplitude", "complex") for fam in ("Morse", "Morlet")]
    plans = {cfg: make(cfg[0], cfg[1], grids[cfg[0]]) for cfg in configs}
    ob = DeviceBuffer(max(p.info["out_bytes"] for p in plans.values()))
    times = collections.defaultdict(list)
    for cfg in configs:
        step_ms(plans[cfg], xb, ob, 3)                # warm-up: tables, clocks
    for rnd in range(4):                              # alternating: A B C D A B C D ...
        for cfg in configs:
            times[cfg] += step_ms(plans[cfg], xb, ob, 5)
    print("## Whole plan, %d ch x %d samples, device-resident step (median of 20, runs alternated)\n" % (C, N))
    print("| wavelet | output | scales | ms / step | min | ms / scale | methods x decimation |")
    print("|---|---|---|---|---|---|---|")
    for cfg in configs:
        p = plans[cfg]
        si = p.scale_info()
        hist = collections.Counter(zip(si["method"].tolist(), si["decimation"].tolist()))
        txt = ", ".join("%s R=%d: %d" % (METHODS[m], r, n) if m == 0 else "%s: %d" % (METHODS[m], n)
                        for (m, r), n in sorted(hist.items(), key=lambda kv: (kv[0][0] != 0, kv[0][1])))
        med = float(np.median(times[cfg]))
        print("| %s | %s | %d | %.2f | %.2f | %.3f | %s; interpolated %d |"
              % (cfg[0] if cfg[0] == "Morse" else "Morlet(w0=%g)" % W0, cfg[1], p.n_freqs, med, min(times[cfg]),
                 med / p.n_freqs, txt, p.info["n_interp"]))
    decs = {cfg: plans[cfg].scale_info() for cfg in configs}
    for p in plans.values():
        p.close()
    print("\n## Per decimation level (a plan of that level's scales alone; synthesis launches, median of 6)\n")
    print("| R | " + " | ".join("%s %s: scales, ms, ms / scale" % cfg for cfg in configs) + " |")
    print("|---|" + "---|" * len(configs))
    all_r = sorted({int(r) for cfg in configs for r, m in zip(decs[cfg]["decimation"], decs[cfg]["method"]) if m == 0})
    for r in all_r:
        cells = []
        for cfg in configs:
            si = decs[cfg]
            f = grids[cfg[0]][(si["decimation"] == r) & (si["method"] == 0)]
            if f.size == 0:
                cells.append("-")
                continue
            p = make(cfg[0], cfg[1], f)
            p.set_profiling(True)
            ts = []
            for _ in range(8):
                p.execute_device(xb, ob)
                t = p.timings()
                ts.append(t["synth_ms"] + t["interp_ms"])
            got = set(p.scale_info()["decimation"].tolist())
            kern = "k_synthi" if p.info["n_interp"] else "k_synth7"
            med = float(np.median(ts[2:]))
            cells.append("%d, %.3f, %.4f (%s%s)" % (f.size, med, med / f.size, kern, "" if got == {r} else ", R %s" % sorted(got)))
            p.close()
        print("| %d | %s |" % (r, " | ".join(cells)))


if __name__ == "__main__":
    main()
