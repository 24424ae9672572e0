"""The detector cases without a device (tests/detector_model.py): the planner still gives every case the levels, shifts,
low cuts and methods tests/test_gpu_detector_matrix.py relies on; the float64 model of k_precision_predict, fed with the
band energies of the float64 FFT, tells the recordings apart as DESIGN.md section 3 says it should and keeps every
prediction clear of the threshold; and the comparison the GPU file makes sees five kinds of damage done to the model at
ten times its bound or more.  A planner change that moves a case fails here, not silently on the device."""
import numpy as np
import pytest

import detector_model as dm

TERM_CASES = [c for c in dm.CASES if c != "A2"]

# (decimation, band_shift) per level; levels with a low cut; the scales on the decimated path (the others must predict 0)
EXPECT = {
    "A": dict(P=1 << 18, levels=[(2 << i, 0) for i in range(9)], cut=list(range(9)), spectral=list(range(24))),
    "F34": dict(P=1 << 16, levels=[(2, 85), (2, 85), (4, 88), (4, 88), (8, 73), (8, 73), (16, 75), (16, 75), (32, 78), (32, 78)],
                cut=[], spectral=list(range(4, 20))),
    "M4": dict(P=1 << 15, levels=[(2, 59), (4, 72), (8, 69), (16, 66), (32, 64)], cut=[], spectral=list(range(2, 16))),
    "M6": dict(P=1 << 16, levels=[(2 << i, 0) for i in range(5)], cut=list(range(5)), spectral=list(range(16))),
    "D": dict(P=1 << 16, levels=[(2 << i, 0) for i in range(6)], cut=list(range(6)), spectral=list(range(3, 20))),
    "A2": dict(P=1 << 17, levels=[(2 << i, 0) for i in range(8)], cut=list(range(8)), spectral=list(range(24))),
}
DAMAGES = ("one_minimum", "own_cut", "no_shift_in_density", "bands_plus_one", "wrong_level")
CAUGHT = 10.0


@pytest.fixture(scope="module")
def models():
    """{case: (plan, tables, P, {recording: model})} on the band energies of the float64 FFT, made once."""
    out = {}
    for case in TERM_CASES:
        plan = dm.make_plan(case)
        tb, P = dm.plan_tables(plan), plan.info["fft_length"]
        out[case] = (plan, tb, P, {r: dm.predict(plan, dm.band_energy(dm.recording(r, dm.CASES[case]["n"]), P), P, tables=tb)
                                   for r in dm.RECORDINGS})
    return out


@pytest.mark.parametrize("case", list(dm.CASES))
def test_every_case_plans_as_listed(case):
    e = EXPECT[case]
    plan = dm.make_plan(case)
    levels = plan.debug_levels()
    assert plan.info["fft_length"] == e["P"]
    assert [(lv["decimation"], lv["band_shift"]) for lv in levels] == e["levels"]
    assert [l for l, lv in enumerate(levels) if lv["low_cut"] > 0] == e["cut"]
    lof = dm.level_of_scale(plan)
    assert np.flatnonzero(lof >= 0).tolist() == e["spectral"]
    assert np.array_equal(plan.scale_info()["method"] == 0, lof >= 0)
    assert sorted(set(lof[lof >= 0].tolist())) == list(range(len(levels)))          # every level has a scale
    # a cut, where there is one, is wide enough to be applied: k1 - k0 >= 1 bin
    for seg in plan.segments():
        assert all(lv["low_cut"] * seg[2] / (4 * np.pi) >= 1 for lv in levels if lv["low_cut"] > 0)
    # the other precision of the GPU file keeps the layout
    auto = dm.make_plan(case, precision="auto")
    assert [(lv["decimation"], lv["band_shift"], lv["low_cut"]) for lv in auto.debug_levels()] == \
        [(lv["decimation"], lv["band_shift"], lv["low_cut"]) for lv in levels]
    if case == "A":
        k1 = [lv["low_cut"] * e["P"] / (2 * np.pi) for lv in levels]
        assert round(k1[0]) == 11523 and round(k1[-1]) == 38
    if case == "F34":
        # two levels per decimation read one x_R: the hook gives both the owner's cut -- none, the bands are shifted.
        # (No plan the planner makes today has two UNSHIFTED levels of one decimation; the own_cut damage below
        # therefore runs on a level split by hand.)
        for a, b in zip(levels[0::2], levels[1::2]):
            assert a["decimation"] == b["decimation"] and a["halo"] < b["halo"] and a["low_cut"] == b["low_cut"] == 0
        assert set(plan.scale_info()["method"][:4].tolist()) == {3}
    if case in ("M4", "D"):
        assert set(plan.scale_info()["method"][:e["spectral"][0]].tolist()) == {1}       # time-domain scales
    if case == "A2":
        assert plan.debug_batches() == [(0, 2), (2, 1)]
        assert plan.segments() == [(3, 58001, 1 << 17), (58007, 116001, 1 << 17), (116010, 146003, 1 << 16)]
        for n_ch in (1, 3):
            assert dm.make_plan(case, n_channels=n_ch).debug_batches() == [(0, 2), (2, 1)]


def test_band_energy_is_the_sum_over_the_band_edges():
    """The bit trick of kernels.h against the edges the model's weights use, and Parseval."""
    P = 1 << 12
    x = dm.recording("white", 3000)
    h = dm.band_energy(x, P)
    X = np.fft.fft(x.astype(np.float64) - x.astype(np.float64).mean(), n=P)
    k = np.arange(1, P // 2)
    for b in (0, 16, 17, 100, 170, 175):
        inside = (k >= dm.BAND_LO[b]) & (k < dm.BAND_HI[b])
        assert abs(h[b] - (np.abs(X[k[inside]]) ** 2).sum()) <= 1e-12 * h.max()
    assert abs(h.sum() - (np.abs(X[1:P // 2]) ** 2).sum()) <= 1e-12 * h.sum()
    assert np.array_equal(dm.band_of(dm.BAND_LO), np.arange(dm.N_BANDS))
    assert np.array_equal(dm.band_of(np.nextafter(dm.BAND_HI.astype(np.float32), np.float32(0))), np.arange(dm.N_BANDS))


def test_model_tells_the_recordings_apart(models):
    for case, (plan, tb, P, by) in models.items():
        spec = tb["level_of"] >= 0
        for r, m in by.items():
            pr = m["predicted"]
            print("%-4s %-10s predicted %.3g .. %.3g, %d of %d over the threshold, left_out decides %d" % (
                case, r, pr[spec].min(), pr[spec].max(), (pr > dm.THRESHOLD).sum(), spec.sum(),
                (m["left_out"] > m["rounding"])[spec].sum()))
            assert np.all(pr[~spec] == 0) and np.all(pr[spec] > 0)
        assert by["pink"]["predicted"].max() < dm.THRESHOLD and by["white"]["predicted"].max() < dm.THRESHOLD, case
        assert (by["line100"]["predicted"] > dm.THRESHOLD).sum() >= 3, case
    a = models["A"][3]
    assert 1.2e-7 < a["pink"]["predicted"].min() and a["pink"]["predicted"].max() < 2.5e-7       # nothing rerouted
    assert (a["line100"]["predicted"] > dm.THRESHOLD).sum() == 22
    assert np.all(a["drift1000"]["left_out"] > a["drift1000"]["rounding"])
    d = models["D"][3]["drift1000"]
    spec = models["D"][1]["level_of"] >= 0
    assert 2 * (d["left_out"] > d["rounding"])[spec].sum() > spec.sum()


def test_no_prediction_within_the_margin_of_the_threshold(models):
    """The verdict tests of the GPU file count predictions over the threshold -- and over twice and half of it: none may
    be so near that the device's float32 sums decide."""
    for case, (plan, tb, P, by) in models.items():
        spec = tb["level_of"] >= 0
        for r, m in by.items():
            for factor in (0.5, 1.0, 2.0):
                near = np.abs(m["predicted"][spec] / (factor * dm.THRESHOLD) - 1).min()
                print("%-4s %-10s nearest to %.1f x threshold: %.3f" % (case, r, factor, near))
                if factor == 1.0:
                    assert near > dm.MARGIN, (case, r, near)
                else:
                    assert near > 10 * dm.REL_TOL, (case, r, factor, near)


def _coverage(models):
    loose = total = 0
    worst = 0.0
    for case, (plan, tb, P, by) in models.items():
        spec = tb["level_of"] >= 0
        for r, m in by.items():
            tol = dm.tolerance(m)
            n = int((tol["abs_part"] > tol["rel_part"])[spec].sum())
            print("%-4s %-10s absolute part above the relative one on %d of %d scales; bound on left_out at most %.2e of "
                  "the prediction" % (case, r, n, spec.sum(), (tol["left_out"][spec] / m["predicted"][spec]).max()))
            loose, total = loose + n, total + int(spec.sum())
            worst = max(worst, float((tol["left_out"][spec] / m["predicted"][spec]).max()))
    return loose, total, worst


def test_bound_on_left_out_is_never_wider_than_the_crude_one(models):
    """The absolute part counts the bands whose weight float32 cannot hold exactly (detector_model.tolerance); with every
    band counted -- 2e-6 sum(h) on E_out, the cruder figure -- the bound would be up to 250 times wider and mostly
    absolute: wherever a level's band CONTAINS the line of 'line100', or a kernel is short enough to answer little to the
    drift of 'drift1000', 122 of the 348 entries.  This bound lies under that one on every entry, and under 1e-4 of what
    is predicted: a term wrong in its fourth digit fails."""
    loose, total, worst = _coverage(models)
    assert worst < 1e-4
    crude = 0
    for case, (plan, tb, P, by) in models.items():
        spec = tb["level_of"] >= 0
        for r, m in by.items():
            tol = dm.tolerance(m)
            assert np.all(tol["left_out"] <= tol["left_out_loose"]) and np.all(m["h_inexact"] <= m["sum_h"])
            assert np.all(m["level_h_inexact"] <= m["sum_h"])
            crude += int((tol["left_out_loose"] - tol["rel_part"] > tol["rel_part"])[spec].sum())
    assert crude == 122


def test_absolute_part_of_the_bound_rarely_exceeds_the_relative_part(models):
    """The condition on coverage: the absolute part of the bound on left_out exceeds the relative part (1e-4 E_out) on at
    most 10 % of the (case, recording, scale) entries.  With the absolute part counted band by band it does on none: the
    interferers of 'line100' and 'drift1000' lie in bands whose weight is exactly 0 or 1 on every level of these cases."""
    loose, total, worst = _coverage(models)
    assert total == 348
    assert loose <= 0.10 * total, (loose, total)


def test_bands_with_inexact_weights_are_the_cut_ones():
    """Which bands carry the absolute part: on case A's level of decimation 8 (P = 2^18: top at bin 32768, low cut from
    k0 = 1574 to k1 = 3149) those centred inside the cut's transition and none else -- the top falls on a band edge."""
    plan = dm.make_plan("A")
    lv = plan.debug_levels()[2]
    P = plan.info["fft_length"]
    w, inexact = dm.level_weights(lv, P, with_inexact=True)
    k1 = lv["low_cut"] * P / (2 * np.pi)
    inside = (dm.BAND_MID > 0.5 * k1) & (dm.BAND_MID < k1)
    assert inexact.sum() == inside.sum() == 16 and np.array_equal(inexact, inside)
    assert np.all((w[~inexact] == 0) | (w[~inexact] == 1)) and np.all((w[inexact] > 0) & (w[inexact] < 1))
    # a shifted level: the two boundaries U and top - U cut a band each, the mirrored copy counts twice below U
    lv = dm.make_plan("M4").debug_levels()[0]
    w, inexact = dm.level_weights(lv, 1 << 15, with_inexact=True)
    assert set(np.unique(w[~inexact]).tolist()) == {0.0, 1.0, 2.0} and 1 <= inexact.sum() <= 2


def _split_level(tb, l):
    """The tables of a plan with level ``l`` split by hand into two levels of one decimation that read one x_R: the
    second takes the upper half of l's scales.  The hook gives both the owner's cut; the second level's own is none."""
    levels = [dict(lv) for lv in tb["levels"]] + [dict(tb["levels"][l])]
    level_of = tb["level_of"].copy()
    mine = np.flatnonzero(level_of == l)
    level_of[mine[len(mine) // 2:]] = len(levels) - 1
    own = [lv["low_cut"] for lv in tb["levels"]] + [0.0]
    return dict(tb, levels=levels, level_of=level_of, own_cut=own)


@pytest.mark.parametrize("damage", DAMAGES)
def test_comparison_sees_damage(models, damage):
    """Each damage moves some term of some (case, recording) by CAUGHT times the bound the GPU file holds the kernel
    to, or more: one minimum over both copies of a shifted band; the level's own low cut for the owner's; the shift
    left out of the density; the bands moved by one; E_level of the next level."""
    best, where = 0.0, None
    for case, (plan, tb, P, by) in models.items():
        if damage == "own_cut":
            if case != "A":
                continue
            tb = _split_level(tb, 3)
        for r in dm.RECORDINGS:
            h = dm.band_energy(dm.recording(r, dm.CASES[case]["n"]), P)
            good = dm.predict(plan, h, P, tables=tb)
            if damage != "own_cut":
                for k in ("rounding", "left_out", "level_energy"):
                    assert np.array_equal(good[k], by[r][k])
            bad = dm.predict(plan, h, P, tables=tb, damage=damage)
            tol = dm.tolerance(good)
            spec = tb["level_of"] >= 0
            for k in ("rounding", "left_out"):
                ratio = (np.abs(bad[k] - good[k])[spec] / np.maximum(tol[k][spec], 1e-300)).max()
                if ratio > best:
                    best, where = ratio, (case, r, k)
    print("%s: %.3g x the bound at %s" % (damage, best, where))
    assert best >= CAUGHT, (damage, best, where)


def test_every_damage_is_seen_in_the_predictions_too(models):
    """... and in max(rounding, left_out), which is all that precision_report() shows of slots other than the first."""
    for damage in DAMAGES:
        best = 0.0
        for case, (plan, tb, P, by) in models.items():
            if damage == "own_cut":
                if case != "A":
                    continue
                tb = _split_level(tb, 3)
            for r in ("line100", "drift1000"):
                h = dm.band_energy(dm.recording(r, dm.CASES[case]["n"]), P)
                good, bad = dm.predict(plan, h, P, tables=tb), dm.predict(plan, h, P, tables=tb, damage=damage)
                spec = tb["level_of"] >= 0
                best = max(best, (np.abs(bad["predicted"] - good["predicted"])[spec] / dm.tolerance(good)["predicted"][spec]).max())
        assert best >= CAUGHT, (damage, best)


def test_segments_of_a2_and_who_decides_each_row():
    """A2 in the model: per (segment, channel) the band energies of the recording minus its global mean on the segment's
    own FFT.  A line at 100 x the spread costs every scale more than a drift at 1000 x does (the drift lies below every
    low cut, and the kernels of these scales hardly answer to it), so the line channel decides every row -- except the
    two rows that hold the line themselves, whose own energy is the line's and whose predicted loss is the smallest of
    all: there the drift channel decides.  The pink channel decides none.  Each by a margin no rounding closes."""
    plan = dm.make_plan("A2", n_channels=3)
    pred = dm.a2_model(plan)                                              # [segment][channel][scale]
    per_channel = pred.max(axis=0)
    who = per_channel.argmax(axis=0)
    f = dm.frequencies("A2")
    print("deciding channel per row:", who.tolist())
    holds_line = (f > 50) & (f < 75)
    assert holds_line.sum() == 2
    assert np.all(who[holds_line] == 2) and np.all(who[~holds_line] == 1)
    ranked = np.sort(per_channel, axis=0)
    assert (ranked[-1] / ranked[-2]).min() > 1.2
    assert np.all(pred[:, 0] < dm.THRESHOLD)
    # the three segments differ: a prediction filed under the wrong segment changes the row's maximum or the block's
    assert np.abs(pred[0] / pred[1] - 1).max() > 100 * dm.REL_TOL and np.abs(pred[2] / pred[1] - 1).max() > 100 * dm.REL_TOL
