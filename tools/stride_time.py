"""Step time of the headline plan (128 ch x 1e6 samples @ 1 kHz x 100 scales, amplitude, device in and out) per
output stride K, the plans' executes alternated in one process (STRIDE_REPS rounds after one warm-up round, medians),
profiling level 2 (events around the synthesis kernels only); then config 5's geometry (48 ch x 18e6 @ 30 kHz x 200
scales) at K = 30 in ONE resident call.  One JSON line.  Per-kernel times: a separate rocprofv3 --kernel-trace --stats
run of this script (STRIDE_C5=0 leaves config 5 out)."""
import json, os, sys, time
sys.path.insert(0, '.')
import numpy as np
from ghost_amd.engine import CwtPlan, DeviceBuffer
from ghost_amd.synthetic import lfp

ks = [int(v) for v in os.environ.get("STRIDE_KS", "1,2,4,5,8,32").split(",")]
reps = int(os.environ.get("STRIDE_REPS", "7"))
fs, C, N, S = 1000.0, 128, 1000000, 100
f = np.geomspace(200.0, 2.0, S)
base = lfp(8, N, fs, seed=1234)
xb = DeviceBuffer(4 * C * N)
for c in range(C):
    xb.upload(base[c % 8], offset_bytes=4 * c * N)
plans, outs = {}, {}
for k in ks:
    plans[k] = CwtPlan(N, C, fs, f, output="amplitude", output_stride=k)
    plans[k].set_profiling(2)
    outs[k] = DeviceBuffer(plans[k].info["out_bytes"])
rows = {k: [] for k in ks}
for it in range(reps + 1):
    for k in ks:
        t0 = time.perf_counter()
        plans[k].execute_device(xb, outs[k])
        dt = (time.perf_counter() - t0) * 1e3
        if it:
            t = plans[k].timings()
            rows[k].append((dt, t["synth_ms"], t["interp_ms"]))
res = {"workload": "128x1e6x100 amplitude, execute_device", "reps": reps, "per_k": {}}
for k in ks:
    a = np.array(rows[k])
    res["per_k"][str(k)] = {"step_ms": round(float(np.median(a[:, 0])), 3), "synth_ms": round(float(np.median(a[:, 1])), 3),
                            "interp_ms": round(float(np.median(a[:, 2])), 3), "out_gb": round(plans[k].info["out_bytes"] / 1e9, 2)}
    if 1 in ks:
        res["per_k"][str(k)]["vs_k1"] = round(res["per_k"][str(k)]["step_ms"] / res["per_k"]["1"]["step_ms"], 3)
for k in ks:
    outs[k].free(); plans[k].close()
xb.free()
if os.environ.get("STRIDE_C5", "1") != "0":
    fs5, C5, N5, S5, k5 = 30000.0, 48, 18000000, 200, 30
    p = CwtPlan(N5, C5, fs5, np.geomspace(500.0, 1.0, S5), output="amplitude", output_stride=k5)
    x5 = lfp(2, N5, fs5, seed=1234)
    xb = DeviceBuffer(4 * C5 * N5)
    for c in range(C5):
        xb.upload(x5[c % 2], offset_bytes=4 * c * N5)
    ob = DeviceBuffer(p.info["out_bytes"])
    ts = []
    for it in range(3):
        t0 = time.perf_counter()
        p.execute_device(xb, ob)
        ts.append((time.perf_counter() - t0) * 1e3)
    res["config5_k30"] = {"out_gb": round(p.info["out_bytes"] / 1e9, 2), "first_ms": round(ts[0], 1),
                          "ms": round(float(np.median(ts[1:])), 1), "segments": len(p.segments())}
    ob.free(); xb.free(); p.close()
print(json.dumps(res))
