"""The front-end cases without a device (tests/level_cases.py): the planner puts every case on the branch it is listed
for, the cases between them reach every kernel the restated dispatch can name, the x_R model is the one
decimated_model.cwt_decimated uses (which is held to the oracle), the comparison catches six kinds of damage done to the
model's own output at ten times a gate or more, and the single-precision reference the tighter gates are taken from stays
inside the project's gates on every recording.  A planner change that moves a case off its branch fails here, not
silently in tests/test_gpu_level_matrix.py."""
import numpy as np
import pytest

import level_cases as lc
from decimated_model import level_input

SLOW_RUNS = [(name, prec) for name in lc.SLOW_FFT_CASES for prec in ("default", "fast")]


def _spectra(name, channel, segment=0):
    """(plan of one channel, P, low bins float64, low bins single, segment input)."""
    plan = lc.make_plan(name, lc.CASES[name]["precisions"][0], n_channels=1)
    p = lc.geometry(plan)[0]
    a, b = lc.epochs_of(name)[segment]
    seg = lc.segment_input(lc.recording(name)[channel], a, b)
    return plan, p, lc.spectrum(seg, p), lc.spectrum(seg, p, single=True), seg


def _factor(got, ref, hard, single):
    """By how much ``got`` misses the gates against ``ref``: the larger of max-error over its hard gate and rms-error
    over RMS_FACTOR times the single-precision reference's.  The GPU tests assert both, so either one catches."""
    mx, rms = lc.compare(got, ref)
    return max(mx / hard, rms / lc.rms_gate(single, ref))


@pytest.mark.parametrize("name", list(lc.CASES))
def test_every_case_plans_onto_its_branch(name):
    c, e = lc.CASES[name], lc.EXPECT[name]
    plan = lc.make_plan(name, c["precisions"][0])
    p, p_store, p1, a, ncol = lc.geometry(plan)
    assert (p, p1, a) == (e["p"], e["p1"], e["a"])
    assert p_store == min(p, 1 << lc.STORE_LOG2) and plan.info["fft_length"] == p
    assert [(lv["decimation"], lv["band_shift"]) for lv in plan.debug_levels()] == e["levels"]
    assert plan.debug_batches() == e["batches"]
    assert set(plan.scale_info()["method"].tolist()) == e["methods"]
    assert ncol == (lc.ROW if 2 in e["methods"] else lc.ROW // 2)
    segs = plan.segments()
    assert [(s[0], s[1]) for s in segs] == [tuple(b) for b in lc.epochs_of(name).tolist()]        # whole epochs, no time blocks
    for s, lv in enumerate(plan.debug_levels(epoch=len(segs) - 1)):
        lead_ne = (segs[-1][0] & 63) + segs[-1][1] - segs[-1][0]
        assert lv["nblk"] == -(-(-(-lead_ne // lv["decimation"])) // lv["hop"])                 # blocks 0 .. nblk - 1
        assert lv["m"] == p // lv["decimation"]
    if name in lc.BLOCK_CASES:
        assert p <= 1 << 16
    if name == "10L":
        assert sorted({s[0] & 63 for s in segs}) == [7, 12, 17, 22, 27, 32]
    if name == "10":
        assert {s[0] & 63 for s in segs} == {0}
    # the other precisions of the case keep the FFT length and the decimations
    for prec in c["precisions"][1:]:
        other = lc.make_plan(name, prec)
        assert lc.geometry(other)[:4] == (p, p_store, p1, a)
        assert all(lv["low_cut"] == 0 for lv in other.debug_levels())
        assert {lv["decimation"] for lv in other.debug_levels()} == {lv["decimation"] for lv in plan.debug_levels()}


def test_block_cases_have_a_ragged_launch():
    """k_block_fft takes sixteen blocks per workgroup: some level must leave a workgroup partly filled."""
    for name in lc.BLOCK_CASES:
        assert any(lv["nblk"] % 16 for lv in lc.make_plan(name).debug_levels()), name


def test_the_table_reaches_every_kernel_of_the_dispatch():
    names = set()
    per_run = {}
    for name, prec in lc.RUNS:
        per_run[(name, prec, False)] = lc.reached(lc.make_plan(name, prec), prec == "fast")
    for name, prec in SLOW_RUNS:
        per_run[(name, prec, True)] = lc.reached(lc.make_plan(name, prec), prec == "fast", slow_fft=True)
    for v in per_run.values():
        names |= v
    every = lc.all_kernel_names()
    assert lc.UNREACHABLE <= every
    assert names == every - lc.UNREACHABLE, (sorted(every - lc.UNREACHABLE - names), sorted(names - every))
    # and each case the kernels it is listed for
    want = {("1", "default"): {"k_fwd64_cols_small", "k_fwd64_rows[half]", "k_fft_rows_fast<+1>"},
            ("1", "fast"): {"k_fft_cols<-1,true>", "k_fft_rows_fast<-1>[half]", "k_fft_rows_fast<+1>"},
            ("2", "default"): {"k_fwd64_rows[mirror]", "k_fft_rows_fast<+1>", "k_fft_rows<+1>", "k_fft_cols<+1,false>"},
            ("3", "default"): {"k_fft_cols<+1,false>", "k_level_small[q>1]"},
            ("4", "default"): {"k_fwd64_cols256_real2", "k_fft_cols256<+1,false>", "k_level_small[q=1]", "k_level_small[q>1]"},
            ("4", "fast"): {"k_fft_cols256_real2", "k_fft_rows_fast<-1>[mirror]"},
            ("5", "default"): {"k_fwd64_colsq_real2<1>", "k_fft_colsq<+1,false,1>"},
            ("5", "fast"): {"k_fft_colsq_real2<1>", "k_fft_rows_fast<-1>[mirror]"},
            ("6", "default"): {"k_fwd64_colsq_real2<2>", "k_fft_colsq<+1,false,2>", "k_level_small[q>1]"},
            ("6", "fast"): {"k_fft_colsq_real2<2>"},
            ("7", "default"): {"k_shift_gather"}, ("8", "default"): {"k_shift_gather", "k_fft_cols<+1,false>"},
            ("9", "default"): {"k_shift_gather", "k_fwd64_rows[full]"},
            ("9", "fast"): {"k_fft_colsq_real2<1>", "k_fft_rows_fast<-1>[full]"},
            ("9s", "fast"): {"k_fft_cols256<-1,true>", "k_fft_rows_fast<-1>[full]"},
            ("11", "default"): {"k_fwd64_colsq_real2<2>", "k_fft_rows_fast<+1>", "k_fft_rows<+1>", "k_level_small[q=1]"}}
    for (name, prec), w in want.items():
        assert w <= per_run[(name, prec, False)], (name, prec, sorted(w - per_run[(name, prec, False)]))
    assert per_run[("2", "fast", True)] == {"k_fft_cols<-1,true>", "k_fft_rows<-1>", "k_fft_rows<+1>", "k_fft_cols<+1,false>"}
    assert per_run[("4", "default", True)] == per_run[("4", "fast", True)] == {
        "k_fft_cols<-1,true>", "k_fft_rows<-1>", "k_fft_rows<+1>", "k_fft_cols<+1,false>", "k_level_small[q=1]", "k_level_small[q>1]"}
    # case 6: k_level_small at its LDS limit, 1024 rows x 8 leading entries x 8 bytes
    lv = [l for l in lc.make_plan("6").debug_levels() if l["decimation"] == 512][0]
    assert lv["m"] == 8192 and min(1024, lv["m"]) * (lv["m"] // 1024) * 8 == 64 * 1024


def test_recordings_tell_channels_apart():
    for name, c in lc.CASES.items():
        x = lc.recording(name)
        assert x.dtype == np.float32 and x.shape == (c["channels"], c["n"])
        assert len({row.tobytes() for row in x}) == c["channels"]
        assert abs(float(x[1].mean()) - lc.OFFSET) < 10.0 and abs(float(x[0].mean())) < 10.0
        tapered = sum(s == 0 for _, s in lc.EXPECT[name]["levels"])
        assert len(lc.tone_angles(name)) == (tapered or int("fast" in c["precisions"]))


@pytest.mark.parametrize("name", ["2", "7", "10L", "9s"])
def test_x_r_model_is_the_one_cwt_decimated_uses(name):
    """level_cases.xr_model fed with the float64 spectrum against decimated_model.level_input (the function
    cwt_decimated takes its x_R from), which carries 1 / R where the engine's x_R carries M: a factor P."""
    seg_i = 3 if name == "10L" else 0
    plan, p, X, _, _ = _spectra(name, 0, seg_i)
    for lv in plan.debug_levels(epoch=seg_i):
        mine = lc.xr_model(X, p, lv)
        theirs = level_input(X, lv) * p
        assert np.abs(mine - theirs).max() <= 1e-12 * np.abs(theirs).max(), (name, lv["decimation"])
    # and from the stored layout, as the GPU test rebuilds the low bins from what it fetched
    _, _, p1, _, ncol = lc.geometry(plan)
    np.testing.assert_array_equal(lc.natural(lc.stored(X, p1, ncol)), X[:p1 * ncol])


@pytest.mark.parametrize("name", list(lc.CASES))
def test_single_precision_reference_and_mutations(name):
    """On the case's own recording: (a) pocketfft in single precision stays inside the project's gates at every stage --
    the inputs themselves do not break them; (b) each mutation of the float64 model misses a gate by CAUGHT or more:
    (i) one mirrored spectrum row left unconjugated, (ii) the low cut moved by one bin, (iii) two channels swapped,
    (iv) the twiddle of one k1 row advanced one step, (v) U off by P1, (vi) one block spectrum taken one sample late."""
    seg_i = {"10": 4, "10L": 4}.get(name, 0)
    plan, p, X, X32, seg = _spectra(name, 0, seg_i)
    _, _, p1, a, ncol = lc.geometry(plan)
    fullband = ncol == lc.ROW
    S, S32 = lc.stored(X, p1, ncol), lc.stored(X32, p1, ncol)
    mx, rms = lc.compare(S32, S)
    print("case %s spectrum: single precision max %.2e rms %.2e" % (name, mx, rms))
    assert mx < lc.GATE_SPECTRUM
    # the channel with the offset, too
    s1 = lc.segment_input(lc.recording(name)[1], *lc.epochs_of(name)[seg_i])
    assert lc.compare(lc.spectrum(s1, p, single=True), lc.spectrum(s1, p))[0] < lc.GATE_SPECTRUM
    # (iii)
    S_other = lc.stored(lc.spectrum(s1, p), p1, ncol)
    assert _factor(S_other, S, lc.GATE_SPECTRUM, S32) >= lc.CAUGHT
    # (i)
    if lc.hermitian(p1, fullband):
        bad = S.copy()
        bad[p1 - 1] = np.conj(bad[p1 - 1])
        f = _factor(bad, S, lc.GATE_SPECTRUM, S32)
        print("  (i) row %d unconjugated: %.1f x" % (p1 - 1, f))
        assert f >= lc.CAUGHT
    xlo = X[:p1 * ncol]
    for l, lv in enumerate(plan.debug_levels(epoch=seg_i)):
        sl = lc.level_slice(xlo, p, lv)
        ref, single = lc.xr_of_slice(sl), lc.xr_of_slice(sl, single=True)
        mx, rms = lc.compare(single, ref)
        print("  level %d R %d: single precision max %.2e rms %.2e" % (l, lv["decimation"], mx, rms))
        assert mx < lc.GATE_XR
        # end to end in single precision
        assert lc.compare(lc.xr_of_slice(lc.level_slice(X32[:p1 * ncol], p, lv), single=True), ref)[0] < lc.GATE_XR
        if l == 0:                                                                                # (iii)
            other = lc.xr_model(lc.natural(S_other), p, lv)
            f = _factor(other, ref, lc.GATE_XR, single)
            print("    (iii) channel 1 for channel 0: %.3g x" % f)
            assert f >= lc.CAUGHT
        if lv["low_cut"] > 0 and np.ptp(lc.low_cut(lv["low_cut"], p, lv["m"])) > 0:                # (ii)
            f = _factor(lc.xr_of_slice(lc.level_slice(xlo, p, lv, taper_roll=1)), ref, lc.GATE_XR, single)
            print("    (ii) low cut one bin late: %.1f x" % f)
            assert f >= lc.CAUGHT, (name, lv["decimation"], f)
        names = lc.level_kernels(p1, lv["decimation"], a, lv["band_shift"])
        if p1 > 1 and not names[0].startswith("k_level_small"):                                  # (iv)
            j1 = p1 - 1
            bad = ref + (np.exp(2j * np.pi * j1 / lv["m"]) - 1) * lc.row_contribution(sl, p1, j1)
            f = _factor(bad, ref, lc.GATE_XR, single)
            print("    (iv) twiddle of row %d one step on: %.1f x" % (j1, f))
            assert f >= lc.CAUGHT, (name, lv["decimation"], f)
        if lv["band_shift"] > 0:                                                                  # (v)
            u = lv["band_shift"] * lv["m"] // lc.BLOCK
            assert u % p1 == 0
            f = _factor(lc.xr_of_slice(lc.level_slice(xlo, p, lv, shift_bins=u + p1)), ref, lc.GATE_XR, single)
            print("    (v) U off by P1: %.3g x" % f)
            assert f >= lc.CAUGHT, (name, lv["decimation"], f)
        if name in lc.BLOCK_CASES:                                                                # (vi)
            xb, xb32 = lc.blocks_model(ref, p, lv), lc.blocks_model(ref, p, lv, single=True)
            assert lc.compare(xb32, xb)[0] < lc.GATE_BLOCKS
            f = _factor(lc.blocks_model(ref, p, lv, late_block=lv["nblk"] // 2), xb, lc.GATE_BLOCKS, xb32)
            print("    (vi) block %d one sample late: %.3g x" % (lv["nblk"] // 2, f))
            assert f >= lc.CAUGHT, (name, lv["decimation"], f)


def test_compare_returns_both_measures():
    ref = np.array([3.0, 4.0j, 0.0, 0.0])
    got = ref + np.array([0.0, 0.0, 0.0, 0.5])
    mx, rms = lc.compare(got, ref)
    assert mx == 0.5 / 4.0 and abs(rms - 0.5 / 5.0) < 1e-15
