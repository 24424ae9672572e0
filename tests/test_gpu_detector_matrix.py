"""The precision detector on the device (GPU): k_precision_predict's two terms and level energies against the float64
model of tests/detector_model.py on every case and recording of that module, the predictor alone (the model is fed
with the device's own band energies); the same bits every run; the two constants; slots and segments beyond the first;
verdicts that follow the predictions; the property the detector exists for -- a row it leaves on the fast path is
inside the gate; and gcwt_debug_check_output, the other piece of code whose job it is to notice.

The bound is derived, not measured (detector_model.tolerance; profiles/detector_model.md has the derivation and the
worst ratios measured against it)."""
import ctypes as C

import numpy as np
import pytest

import detector_model as dm
from conftest import rel_err
from oracle import ghost_oracle as orc

pytestmark = pytest.mark.gpu

TERM_CASES = [c for c in dm.CASES if c != "A2"]
RUNS = [(c, r) for c in TERM_CASES for r in dm.RECORDINGS]
GATE = 1e-5
BAND_TOL = 2e-5                 # what test_band_energies_of_the_detector_are_those_of_the_spectrum holds the band sums to


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _execute(case, x, precision="high", n_channels=1):
    plan = dm.make_plan(case, precision=precision, n_channels=n_channels)
    out = plan.execute(np.atleast_2d(x))
    return plan, out


@pytest.fixture(scope="module")
def watched():
    """{(case, recording): (plan, terms, predicted)} of precision = 'high': watched, nothing rerouted.  One execute
    each, shared by the tests below."""
    res = {}
    for case, r in RUNS:
        plan, _ = _execute(case, dm.recording(r, dm.CASES[case]["n"]))
        rep = plan.precision_report()
        assert rep["watched"] and rep["rerouted"] == 0
        res[(case, r)] = (plan, plan.debug_precision_terms(), rep["predicted"].copy())
    return res


@pytest.fixture(scope="module")
def tables():
    return {}


def _tables(cache, case, plan):
    if case not in cache:
        cache[case] = dm.plan_tables(plan)
    return cache[case]


@pytest.mark.parametrize("case, recording", RUNS)
def test_terms_are_those_of_the_model(watched, tables, case, recording):
    plan, terms, predicted = watched[(case, recording)]
    tb = _tables(tables, case, plan)
    P = plan.info["fft_length"]
    model = dm.predict(plan, terms["band_energy"].astype(np.float64), P, tables=tb)
    tol = dm.tolerance(model)
    spec = tb["level_of"] >= 0
    worst = {}
    for k in ("rounding", "left_out", "level_energy"):
        got = terms[k].astype(np.float64)
        sel = spec if k != "level_energy" else np.ones(len(tb["levels"]), bool)
        ratio = np.abs(got - model[k])[sel] / tol[k][sel]
        worst[k] = ratio.max()
        print("%-4s %-10s %-12s worst |kernel - model| / bound %.4f (scale or level %d: kernel %.6g model %.6g)" % (
            case, recording, k, ratio.max(), np.flatnonzero(sel)[ratio.argmax()], got[sel][ratio.argmax()],
            model[k][sel][ratio.argmax()]))
    assert max(worst.values()) <= 1.0, worst
    # scales off the decimated path predict nothing, to the bit; the others something
    assert np.all(_bits(predicted)[~spec] == 0) and np.all(_bits(terms["rounding"])[~spec] == 0)
    assert np.all(_bits(terms["left_out"])[~spec] == 0)
    assert np.all(predicted[spec] > 0)
    # one channel, one segment: the report is the larger term, the kernel's own fmaxf
    assert np.array_equal(_bits(predicted), _bits(np.maximum(terms["rounding"], terms["left_out"])))


@pytest.mark.parametrize("case", TERM_CASES)
def test_same_bits_every_time(watched, case):
    """Fixed order of every sum, and atomicMin on non-negative floats does not depend on order."""
    plan, terms, predicted = watched[(case, "line100")]
    x = dm.recording("line100", dm.CASES[case]["n"])
    for _ in range(2):
        plan.execute(x[None, :])
        again = plan.debug_precision_terms()
        for k in ("rounding", "left_out", "level_energy", "band_energy"):
            assert np.array_equal(_bits(again[k]), _bits(terms[k])), k
        assert np.array_equal(_bits(plan.precision_report()["predicted"]), _bits(predicted))


@pytest.mark.parametrize("case", TERM_CASES)
def test_the_two_constants(watched, option, case):
    """Twice kappa doubles the rounding term and leaves the other's bits alone, twice the out-of-band constant the
    converse: multiplying by two is exact, and E_s and the rest do not change."""
    _, terms, predicted = watched[(case, "drift1000")]
    x = dm.recording("drift1000", dm.CASES[case]["n"])
    option("auto_kappa_ppb", 320)
    plan, _ = _execute(case, x)
    t = plan.debug_precision_terms()
    assert np.array_equal(_bits(t["rounding"]), _bits(2.0 * terms["rounding"]))
    assert np.array_equal(_bits(t["left_out"]), _bits(terms["left_out"]))
    assert np.array_equal(_bits(plan.precision_report()["predicted"]), _bits(np.maximum(t["rounding"], t["left_out"])))
    option("auto_kappa_ppb", None)
    option("auto_oob_ppt", 50000)
    plan, _ = _execute(case, x)
    t = plan.debug_precision_terms()
    assert np.array_equal(_bits(t["rounding"]), _bits(terms["rounding"]))
    assert np.array_equal(_bits(t["left_out"]), _bits(2.0 * terms["left_out"]))
    assert np.array_equal(_bits(t["level_energy"]), _bits(terms["level_energy"]))


def test_slots_and_segments():
    """A2: three channels (pink, line, drift), two segments in one batch and a third in a batch of its own.  The report
    is the maximum over (segment, channel): bit for bit that of three one-channel plans, and the model's within its
    bound plus the band sums'.  The model says which channel decides a row (tests/test_detector_cases_cpu.py pins it:
    the line channel everywhere but on the two rows that hold the line, where the drift channel does): a prediction
    filed under the wrong channel or segment cannot keep all of this intact."""
    x = dm.a2_recording()
    plan, _ = _execute("A2", x, n_channels=3)
    got = plan.precision_report()["predicted"]
    ones = []
    singles = []
    for c in range(3):
        p1, _ = _execute("A2", x[c])
        ones.append(p1.precision_report()["predicted"].copy())
        singles.append(p1)
    ones = np.stack(ones)
    assert np.array_equal(_bits(got), _bits(ones.max(axis=0)))
    model, tol = dm.a2_model(plan, with_tolerance=True)                 # [segment][channel][scale]
    bound = (tol + BAND_TOL * model).max(axis=(0, 1))
    ratio = np.abs(got - model.max(axis=(0, 1))) / bound
    print("A2 report against the model's maximum: worst / bound %.3f" % ratio.max())
    assert ratio.max() <= 1.0
    # ... and channel by channel (the one-channel plans: maximum over the segments)
    for c in range(3):
        b = (tol[:, c] + BAND_TOL * model[:, c]).max(axis=0)
        r = np.abs(ones[c] - model[:, c].max(axis=0)) / b
        print("A2 channel %d alone: worst / bound %.3f" % (c, r.max()))
        assert r.max() <= 1.0
    who = model.max(axis=0).argmax(axis=0)
    assert set(who.tolist()) == {1, 2}
    assert np.array_equal(ones.argmax(axis=0), who)
    assert np.array_equal(_bits(got), _bits(ones[who, np.arange(plan.n_freqs)]))
    # slot 0 of the last batch is (segment 2, channel 0): the terms hook follows
    t, t0 = plan.debug_precision_terms(), singles[0].debug_precision_terms()
    for k in ("rounding", "left_out", "level_energy", "band_energy"):
        assert np.array_equal(_bits(t[k]), _bits(t0[k])), k
    b20 = tol[2, 0] + BAND_TOL * model[2, 0]
    assert (np.abs(np.maximum(t["rounding"], t["left_out"]) - model[2, 0]) / b20).max() <= 1.0
    # a block request inside the second epoch: that segment alone
    a, b, _ = plan.segments()[1]
    plan.execute_block(x, a + 1000, b - a - 2000)
    blk = plan.precision_report()["predicted"]
    bb = (tol[1] + BAND_TOL * model[1]).max(axis=0)
    r = np.abs(blk - model[1].max(axis=0)) / bb
    print("A2 block of the second epoch: worst / bound %.3f" % r.max())
    assert r.max() <= 1.0
    blk_ones = []
    for c in range(3):
        singles[c].execute_block(x[c], a + 1000, b - a - 2000)
        blk_ones.append(singles[c].precision_report()["predicted"].copy())
    assert np.array_equal(_bits(blk), _bits(np.stack(blk_ones).max(axis=0)))
    assert not np.array_equal(_bits(blk), _bits(got))


@pytest.mark.parametrize("case, recording", RUNS)
def test_verdicts_follow_predictions(watched, option, case, recording):
    """precision = 'auto': as many scales are made again as predictions lie over the threshold, at the default, at twice
    and at half of it; the predictions are those of 'high', bit for bit (the CPU file keeps them clear of all three
    thresholds)."""
    _, _, predicted = watched[(case, recording)]
    x = dm.recording(recording, dm.CASES[case]["n"])
    for ppb in (None, 3000, 750):
        option("auto_threshold_ppb", ppb)
        plan, out = _execute(case, x, precision="auto")
        rep = plan.precision_report()
        assert np.array_equal(_bits(rep["predicted"]), _bits(predicted))
        want = int((predicted > np.float32(1e-9) * np.float32(ppb or 1500)).sum())
        print("%-4s %-10s threshold %d ppb: %d rerouted" % (case, recording, ppb or 1500, rep["rerouted"]))
        assert rep["rerouted"] == want, (ppb, rep["rerouted"], want)
        assert np.isfinite(out).all()


# ---- the safety property ---------------------------------------------------------------------------------------------
SAFETY = [(f, a) for f in (60.0, 17.0, 141.0) for a in (30.0, 100.0, 300.0)]


@pytest.fixture(scope="module")
def safety_runs():
    """Case D's plan, precision = 'high' (the fast path's rows come back), pink plus a line: per (frequency, amplitude)
    the predictions and the rows' errors against the oracle.  One plan, nine executes, nine oracle transforms."""
    plan = dm.make_plan("D")
    f = dm.frequencies("D")
    res = {}
    for freq, amp in SAFETY:
        x = dm.line(dm.CASES["D"]["n"], amp, freq)
        out = plan.execute(x[None, :])[0]
        ref = np.abs(orc.cwt_complex(x.astype(np.float64), dm.FS, f, n_threads=8))
        res[(freq, amp)] = (plan.precision_report()["predicted"].copy(), rel_err(out, ref))
    return res, dm.level_of_scale(plan) >= 0


@pytest.mark.parametrize("freq, amp", SAFETY)
def test_rows_left_on_the_fast_path_are_inside_the_gate(safety_runs, freq, amp):
    runs, spec = safety_runs
    predicted, err = runs[(freq, amp)]
    f = dm.frequencies("D")
    print("line %g Hz at %g x the spread: row, Hz, predicted, measured" % (freq, amp))
    for i in np.flatnonzero(spec):
        print("  %2d %7.2f %.3g %.3g%s" % (i, f[i], predicted[i], err[i], "" if predicted[i] <= dm.THRESHOLD else "  (rerouted by 'auto')"))
    kept = spec & (predicted <= np.float32(dm.THRESHOLD))
    assert kept.any()
    assert err[kept].max() < GATE, (np.flatnonzero(kept)[err[kept].argmax()], err[kept].max())
    assert err[~spec].max() < GATE                                        # the time-domain rows, whatever the line


# ---- gcwt_debug_check_output -----------------------------------------------------------------------------------------
N_CH, DISTINCT, N_ROWS = 5, 2, 3
POS_INF, NEG_INF, QNAN, SNAN, NEG_NAN = 0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001, 0xFFC00001
NONFINITE = (POS_INF, NEG_INF, QNAN, SNAN, NEG_NAN)


def _check(buf, pitch, n_valid, rows=N_ROWS, n_ch=N_CH, distinct=DISTINCT):
    from ghost_amd._lib import lib
    bad, diff = C.c_int64(-1), C.c_int64(-1)
    rc = lib.gcwt_debug_check_output(buf.ptr if buf is not None else None, pitch, n_valid, rows, n_ch, distinct,
                                     C.byref(bad), C.byref(diff))
    return rc, bad.value, diff.value


def _planted(n_valid, pitch):
    """(bits [C][S][pitch], non-finite count, mismatch count): channel c equals channel c % 2, NaN in the padding, and
    at the first and last valid column, at multiples of 256 and of 64 * 256 and at the kernel's own grid stride a
    rotation of seven plants whose counts are known by construction."""
    rng = np.random.default_rng(n_valid)
    base = rng.standard_normal((DISTINCT, N_ROWS, pitch)).astype(np.float32).view(np.uint32)
    a = np.stack([base[c % DISTINCT] for c in range(N_CH)]).copy()
    a[:, :, n_valid:] = QNAN
    stride = 256 * min(64, (n_valid + 4095) // 4096)
    cols = sorted({c for c in (0, n_valid - 1, 255, 256, 257, 512, 4095, 4096, stride - 1, stride, 2 * stride, 16384, 16385,
                               32768, 65536, 65537) if 0 <= c < n_valid})
    bad = diff = 0
    for i, (col, s) in enumerate((col, s) for col in cols for s in range(N_ROWS)):
        v = NONFINITE[i % len(NONFINITE)]
        kind = i % 7
        if kind == 0:                      # a distinct channel alone: both of its twins differ from it
            a[0, s, col] = v
            bad, diff = bad + 1, diff + 2
        elif kind == 1:                    # a tiled channel alone
            a[3, s, col] = v
            bad, diff = bad + 1, diff + 1
        elif kind == 2:                    # the same bits in a channel and its twin: twice non-finite, no mismatch
            a[1, s, col] = a[3, s, col] = v
            bad += 2
        elif kind == 3:                    # NaN against another NaN: the check is on bits
            a[0, s, col], a[4, s, col] = QNAN, SNAN
            bad, diff = bad + 2, diff + 2
        elif kind == 4:                    # subnormals are finite
            a[2, s, col] = (0x00000001, 0x807FFFFF)[i % 2]
            a[0, s, col] = 0x00000002
            a[4, s, col] = 0x00000002
            diff += 1
        elif kind == 5:                    # -0.0 against +0.0
            a[1, s, col], a[3, s, col] = 0x00000000, 0x80000000
            diff += 1
        else:                              # the largest finite value everywhere: nothing to count
            a[0, s, col] = a[2, s, col] = a[4, s, col] = 0x7F7FFFFF
    return a, bad, diff


@pytest.mark.parametrize("n_valid", [1, 255, 256, 4097, 70001])
@pytest.mark.parametrize("padded", [False, True])
def test_check_output_counts_what_was_planted(n_valid, padded):
    from ghost_amd.engine import DeviceBuffer
    pitch = (n_valid + 31) & ~31 if padded else n_valid
    if padded and pitch == n_valid:
        pitch += 32
    a, bad, diff = _planted(n_valid, pitch)
    # the counts by construction against a plain count over the array
    valid = a[:, :, :n_valid]
    assert bad == int(((valid & 0x7F800000) == 0x7F800000).sum())
    assert diff == int(sum((valid[c] != valid[c % DISTINCT]).sum() for c in range(DISTINCT, N_CH)))
    assert n_valid == 1 or (bad > 0 and diff > 0)
    buf = DeviceBuffer(a.nbytes)
    try:
        buf.upload(a)
        assert _check(buf, pitch, n_valid) == (0, bad, diff)
        # every channel its own: nothing to compare
        assert _check(buf, pitch, n_valid, distinct=N_CH) == (0, bad, 0)
        assert _check(buf, pitch, n_valid, distinct=N_CH + 2) == (0, bad, 0)
        # clean twins: the planted array's distinct channels tiled again
        clean = np.stack([a[c % DISTINCT] for c in range(N_CH)])
        buf.upload(clean)
        rc, bad_clean, diff_clean = _check(buf, pitch, n_valid)
        cv = clean[:, :, :n_valid]
        assert (rc, bad_clean, diff_clean) == (0, int(((cv & 0x7F800000) == 0x7F800000).sum()), 0)
        # finite everywhere: both counts zero
        buf.upload(np.where((clean & 0x7F800000) == 0x7F800000, np.uint32(0x3F800000), clean).astype(np.uint32))
        assert _check(buf, pitch, n_valid) == (0, 0, 0)
    finally:
        buf.free()


def test_check_output_refuses_bad_arguments():
    from ghost_amd._lib import ERR_INVALID, lib
    from ghost_amd.engine import DeviceBuffer
    buf = DeviceBuffer(4 * 64 * N_CH * N_ROWS)
    try:
        buf.zero()
        bad, diff = C.c_int64(0), C.c_int64(0)
        args = (64, 64, N_ROWS, N_CH, DISTINCT)
        assert lib.gcwt_debug_check_output(None, *args, C.byref(bad), C.byref(diff)) == ERR_INVALID
        assert lib.gcwt_debug_check_output(buf.ptr, *args, None, C.byref(diff)) == ERR_INVALID
        assert lib.gcwt_debug_check_output(buf.ptr, *args, C.byref(bad), None) == ERR_INVALID
        assert _check(buf, 63, 64)[0] == ERR_INVALID                          # pitch < n_valid
        assert _check(buf, 64, 64, rows=13108, n_ch=5)[0] == ERR_INVALID      # 65540 rows: more than one grid holds
        assert _check(buf, 64, 64) == (0, 0, 0)
    finally:
        buf.free()
