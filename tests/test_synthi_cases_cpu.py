"""The cases of tests/synthi_cases.py on the host: the planner takes each of them to the branch of k_synthi it is there
for, and the float64 model agrees with the oracle on every row.  A change to the planner or to work_items.cpp's cut that moves
a case off its branch fails here, not silently on the GPU.  No device."""
import numpy as np
import pytest

import synthi_cases as sc
from conftest import rel_err


@pytest.fixture(scope="module")
def reached():
    """{case: branches(plan)} -- planning only."""
    return {name: sc.branches(sc.make_plan(name)) for name in sc.CASES}


def _levels(reached):
    return [(name, b) for name, br in reached.items() for b in br.values()]


@pytest.mark.parametrize("name", list(sc.CASES))
def test_case_reaches_its_designs(name):
    """(q, I, taps) of every level, the refused ones included, as pinned in synthi_cases.DESIGNS."""
    plan = sc.make_plan(name)
    assert sc.designs(plan) == sc.DESIGNS[name]
    for d in plan.debug_interp()["levels"]:
        if d is not None:
            assert d["coef"].shape == (2, d["factor"], 8) and 0 < d["err_bound"] <= 2e-7
    on, refused = sc.interpolated_rows(plan)
    assert plan.info["n_interp"] == on.size
    # complex output never interpolates
    c = sc.CASES[name]
    from ghost_amd.engine import CwtPlan
    assert CwtPlan(c["n"], 1, c["fs"], c["f"], gamma=c["gamma"], beta=c["beta"], epoch_bounds=c["epochs"],
                   output="complex").info["n_interp"] == 0


def test_layouts():
    """One segment, two epochs of one batch whose bounds and gap are multiples of neither 4 nor 64, two time blocks."""
    assert sc.make_plan("B").segments() == [(0, 1 << 17, 1 << 18)]
    assert sc.make_plan("C").segments() == [(0, 1 << 21, 1 << 22)]
    b2 = sc.make_plan("B2")
    assert b2.segments() == [(3, 58001, 1 << 17), (58007, 116001, 1 << 17)] and b2.debug_batches() == [(0, 2)]
    (a0, a1), (b0, b1) = sc.CASES["B2"]["epochs"]
    assert all(v % 4 and v % 64 for v in (a0, a1, b0, b1, b0 - a1))
    d = sc.make_plan("D")
    assert [p for _, _, p in d.segments()] == [1 << 22, 1 << 22] and d.debug_batches() == [(0, 2)]
    assert d.segments()[0][1] == d.segments()[1][0]                       # two time blocks of the one epoch
    assert all(sc.CASES[n]["n"] <= 1 << 21 for n in sc.CASES if n != "D") and sc.CASES["D"]["n"] == 1 << 22


def test_cases_cover_every_branch(reached):
    lv = _levels(reached)
    assert {b["q"] for _, b in lv} == {2, 4, 8, 16}
    assert {b["taps"] for _, b in lv if b["decimation"] >= 32} == {6, 8}
    assert {b["taps"] for _, b in lv if b["q"] == 2} == {8}
    assert {b["lgi4"] for _, b in lv} == set(range(1, 9))
    assert {b["lgi4"] for n, b in lv if n == "C"} >= {7, 8}                # the class depends on wt mod 4 (lgi4 > 6)
    # q = 16: one scale per pass, one z slot, one block per segment
    (q16,) = [b for _, b in lv if b["q"] == 16]
    assert q16["decimation"] == 16384 and q16["nblk"] == 1 and all(c["ns"] == 1 and c["nb"] == 1 for c in q16["cut"].values())
    # parities: a level of both with the coefficient table switched at least twice along the walk -- under the default
    # cut and under a forced one --, and a level of one parity
    assert any(len(set(b["parities"])) == 2 and b["cut"][None]["switches"] >= 2 for _, b in lv)
    assert any(len(set(b["parities"])) == 2 and b["cut"][1]["switches"] >= 2 for n, b in lv if n in sc.CUT_CASES)
    assert any(len(set(b["parities"])) == 1 and len(b["parities"]) > 1 for _, b in lv)
    # ragged last passes and groups
    for opt in (None, 0, 1, 2):
        assert any(b["cut"][opt]["ragged"] and b["cut"][opt]["n_pass"] > 1 for n, b in lv if n in sc.CUT_CASES), opt
    assert any(len(b["rows"]) < b["cut"][None]["ns"] for _, b in lv)
    for opt in (1, 2):
        assert any(b["cut"][opt]["nb"] == 1 << opt and b["cut"][opt]["ragged_blocks"] for n, b in lv if n in sc.CUT_CASES), opt
    # the clamp (q << lgnb) <= 16
    assert any(b["cut"][2]["lgnb"] < 2 for _, b in lv) and any(b["cut"][2]["lgnb"] == 2 for _, b in lv)
    # shifted bands, long halos, two levels of one decimation
    assert any(b["shift"] > 0 and b["halo"] > 32 for n, b in lv if n == "F34")
    assert all(b["shift"] > 0 for n, b in lv if n in ("F34", "F28"))
    r34 = [b["decimation"] for n, b in lv if n == "F34"]
    assert len(r34) > len(set(r34))
    # a level the design refuses beside interpolated ones
    plan = sc.make_plan("E")
    on, refused = sc.interpolated_rows(plan)
    assert on.size and refused.size and set(plan.scale_info()["decimation"][refused]) == {16}


def test_cut_reaches_shared_passes_and_runs(reached):
    """Items of several parts (a pass's wave-tasks shared among workgroups), items that start after the level's first
    pass, a level walked in a single pass by one item per block group -- from the restated cut (synthi_cases.items)."""
    for name in ("B", "C", "D"):
        its = [it for b in reached[name].values() for it in b["items"]]
        assert any(it["parts"] > 1 for it in its), name
        assert any(it["pass0"] > 0 for it in its), name
    assert any(it["parts"] > 1 and it["pass0"] > 0 for b in reached["C"].values() for it in b["items"])
    single = [b for b in reached["B"].values() if all(it["parts"] == 1 and it["pass0"] == 0 for it in b["items"])]
    assert single and all(b["cut"][None]["n_pass"] == 1 for b in single)
    for name, b in _levels(reached):
        for it in b["items"]:
            assert 0 <= it["lo"] < it["hi"] <= it["wps"] and it["lo"] % 4 == 0, (name, it)
        # the parts of a (block group, pass run) tile the wave-tasks
        groups = {}
        for it in b["items"]:
            groups.setdefault((it["blk0"], it["pass0"]), []).append((it["lo"], it["hi"]))
        for spans in groups.values():
            spans.sort()
            assert spans[0][0] == 0 and spans[-1][1] == b["items"][0]["wps"]
            assert all(a[1] == c[0] for a, c in zip(spans[:-1], spans[1:]))
    # the channel count moves `target`, hence the parts, of case C (what the 40-channel GPU test relies on)
    t1, t40 = sc.items(sc.make_plan("C"))[1], sc.items(sc.make_plan("C", n_channels=40))[1]
    assert t1 == 1 << 19 and t40 == 2 << 20
    top1 = max(it["parts"] for it in sc.items(sc.make_plan("C"))[0])
    top40 = max(it["parts"] for it in sc.items(sc.make_plan("C", n_channels=40))[0])
    assert top40 < top1


def test_host_gain_is_the_models_gain():
    """``debug_exact_gain`` (what the model takes G from for kernels of a million taps) against the NumPy ``exact_gain``
    on short scales, on the level's own grid, shifted band included."""
    from decimated_model import exact_gain, level_of_scale
    from oracle import ghost_oracle as orc
    for name in ("B", "F34"):
        c, plan = sc.CASES[name], sc.make_plan(name)
        si, levels, lof = plan.scale_info(), plan.debug_levels(), level_of_scale(plan)
        om = orc.hz_to_rad(c["f"], c["fs"])
        for i in sc.interpolated_rows(plan)[0][:4]:
            lv = levels[lof[i]]
            k = np.arange(256) - lv["band_shift"]
            ref = exact_gain(2 * np.pi * k / (256 * lv["decimation"]), om[i], int(si["length"][i]), c["gamma"], c["beta"])
            got = plan.debug_exact_gain(i, k, 256 * lv["decimation"])
            assert np.abs(got - ref).max() < 1e-12 * np.abs(ref).max(), (name, i)


@pytest.mark.parametrize("name", sc.MODELLED)
def test_model_matches_oracle_on_every_row(name):
    """Every row of the case, every sample (the gaps of the two-epoch case included: zero in both)."""
    err = rel_err(sc.model(name), sc.oracle(name))
    print(name, "model against oracle, worst row %.3g" % err.max())
    assert err.shape == (len(sc.CASES[name]["f"]),) and err.max() < sc.MODEL_CPU, err


@pytest.mark.parametrize("split_r", (0, 64))
@pytest.mark.parametrize("lgnb", (None, 0, 1, 2))
@pytest.mark.parametrize("name,n_channels", [(n, 1) for n in sc.CASES] + [("C", 40)])
def test_restated_cut_is_the_librarys(option, name, n_channels, lgnb, split_r):
    """``synthi_cases.items`` -- what the GPU matrix places its windows by -- against the items the library cuts
    (``debug_work_items``: what the upload sends), field by field, under every forced number of blocks per workgroup
    and with one launch or two.  The upload orders the list: the levels below interp_split_r first, then by output
    bytes, largest first, ties in the order of the cut.  Case C at 1 and at 40 channels: `target` halved and not."""
    if lgnb is not None:
        option("interp_lgnb", lgnb)
    option("interp_split_r", split_r)
    plan = sc.make_plan(name, n_channels=n_channels)
    its, _ = sc.items(plan, lgnb)
    levels, di = plan.debug_levels(), plan.debug_interp()["levels"]

    def out_bytes(it):
        lv, q = levels[it["level"]], di[it["level"]]["q"]
        nb = 1 << sc.clamp_lgnb(lv["decimation"], q, lgnb)
        pass_bytes = (sc.K_COLS // (q * nb)) * nb * lv["hop"] * lv["decimation"] * 4
        return it["n_pass"] * pass_bytes * (it["hi"] - it["lo"]) // max(1, it["wps"])
    its = sorted(its, key=lambda it: (it["decimation"] >= split_r, -out_bytes(it)))
    got = plan.debug_work_items("interp")
    assert got["items"].size == len(its) > 0
    for field in ("level", "blk0", "pass0", "n_pass", "lo", "hi"):
        assert got["items"][field].tolist() == [it[field] for it in its], (name, field)
    assert got["split"] == sum(it["decimation"] < split_r for it in its)
    if name in ("B", "E", "F28"):                         # levels on both sides of R = 64
        assert (0 < got["split"] < len(its)) == (split_r == 64)
