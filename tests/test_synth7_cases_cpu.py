"""The cases of tests/synth7_cases.py on the host: the planner takes each of them to the branch of k_synth7 it is there
for, and the float64 model of the stage -- fed the float64 level input instead of a device buffer -- reproduces the
whole-path models and agrees with the oracle on every row.  A change to the planner that moves a case off its branch
fails here, not silently on the GPU.  No device."""
import numpy as np
import pytest

import morlet_model
import synth7_cases as s7
from conftest import rel_err
from decimated_model import cwt_decimated

# stage_model (all blocks at once, the R phases as one zero-padded inverse transform) against cwt_decimated /
# morlet_model.cwt_decimated (block by block, explicit polyphase twiddles), both float64 from the same level input:
# worst row measured 3.0e-15 over the cases without a band shift (case W, R = 4096: one inverse transform of 2^20 points;
# 6e-16 elsewhere) -> 10 x.  Shifted bands (M4, HW): 3.8e-12 and 3.0e-12 -- cwt_decimated takes the carrier's
# phase 2 pi shift (b hop - halo + m) / 256 as it stands, up to 3e4 radians, 3e4 x 1.1e-16 of rounding; the stage model
# reduces shift n mod 256 R in integers first -> 10 x 3.8e-12.
MODEL_NOISE = 10 * 3.0e-15
MODEL_NOISE_SHIFTED = 10 * 3.8e-12
MORLET_CPU = 2.5e-6             # morlet_cases.MODEL_TOL


@pytest.fixture
def plan_of(option):
    def make(name, output="complex", n_channels=None):
        for k, v in s7.plan_options(name, output).items():
            option(k, v)
        plan = s7.make_plan(name, output, n_channels)
        for k in s7.plan_options(name, output):
            option(k, None)
        return plan
    return make


def _k7_rows(plan):
    return np.concatenate([lv["rows"] for lv in s7.levels(plan) if lv["kernel"].startswith("k_synth7")])


@pytest.mark.parametrize("name", list(s7.CASES))
def test_level_table(plan_of, name):
    """(R, halo, hop, blocks, shift, scales, n_plain, kernel) of every level that holds scales, for every output mode
    the case runs in; nothing interpolated; the lists' order: odd kernel lengths first."""
    c = s7.CASES[name]
    for output in c["outputs"]:
        plan = plan_of(name, output)
        assert s7.table(plan) == s7.EXPECT[name], (name, output)
        assert plan.info["n_interp"] == 0
        si = plan.scale_info()
        for lv in s7.levels(plan):
            assert lv["scales"].size <= 256
            assert not lv["j_hi"].any()                   # the windows are set on the device
            if c["w0"] is None:
                odd = si["length"][lv["rows"]] % 2 == 1
                assert odd[:lv["n_plain"]].all() and not odd[lv["n_plain"]:].any()
            else:
                assert lv["n_plain"] == lv["scales"].size
    rows = _k7_rows(plan)
    if name != "HW":
        assert rows.size == len(c["f"])                   # every row is k_synth7's
    else:
        assert set(plan.scale_info()["method"][np.setdiff1d(np.arange(len(c["f"])), rows)]) == {3}


def _family(fam, plan_of, output="complex"):
    return [(n, lv) for n in s7.CASES if s7.FAMILY[n] == fam and output in s7.CASES[n]["outputs"]
            for lv in s7.levels(plan_of(n, output))]


def test_case_a_reaches_every_chunk_and_ramp_position(plan_of):
    for output, max_r in (("amplitude", 8), ("power", 8), ("complex", 32)):
        lv = [l for _, l in _family("A", plan_of, output)]
        assert {l["decimation"] for l in lv} == {2, 4, 8, 16, 32} - set(range(max_r + 1, 33))
        sizes = {int(l["scales"].size) for l in lv}
        assert sizes >= {1, 7, 8, 9, 16, 17}, output
        where = {(s7.ramp_position(l["scales"].size, l["n_plain"]), int(l["scales"].size)) for l in lv}
        assert {w for w, _ in where} == {"start", "never", "chunk", "inside"}
        assert ("chunk", 9) in where                                  # the ramp on the level's last scale, alone in its chunk
        assert any(w == "chunk" and n > 9 for w, n in where)          # ... on the second chunk's first scale, more behind
        assert any(l["n_plain"] == 8 for l in lv)
        # first, interior and ragged last group of blocks in both column builds (and under synth7_narrow_r)
        for l in lv:
            for cols in (16, 32):
                groups, ragged = s7.block_groups(l, cols)
                assert groups > 2, (l["decimation"], cols)
            if l["decimation"] <= 16:                     # (above, a workgroup is one block: no group is ragged)
                assert s7.block_groups(l, 32)[1], l["decimation"]
        assert any(s7.block_groups(l, 16)[1] for l in lv)
    # every first-layer window, predicted from the float64 response (the device's own are read on the GPU)
    seen = set()
    for n in ("A1", "A2"):
        plan = plan_of(n, "amplitude")
        for l in s7.levels(plan):
            seen |= set(s7.predicted_j_hi(n, plan, l).tolist())
    assert seen == set(range(9, 17))


def test_case_a256_is_the_largest_level(plan_of):
    for name, n in (("A256", 256), ("A255", 255)):
        (lv,) = s7.levels(plan_of(name))
        assert lv["scales"].size == n and lv["n_plain"] == 127 and lv["n_plain"] // 8 == 15 and lv["n_plain"] % 8
        assert -(-n // 8) == 32 and lv["nblk"] == 8


def test_case_m_reaches_the_complex_gain_chunks(plan_of):
    for name, shifted in (("M6", False), ("M4", True)):
        lv = s7.levels(plan_of(name))
        assert {int(l["scales"].size) for l in lv} == {1, 3, 4, 5, 8, 9}
        assert all((l["band_shift"] > 0) == shifted and l["n_plain"] == l["scales"].size for l in lv)
    assert any(l["halo"] > 32 for l in s7.levels(plan_of("M4")))       # rows 2 / 13 lane-wise with complex gains


def test_case_w_reaches_the_phase_tiles(plan_of):
    plan = plan_of("W")
    lv = s7.levels(plan)
    assert plan.segments() == [(0, 1 << 18, 1 << 20)]
    assert [s7.phase_tiles(l["decimation"], 32) for l in lv] == [2, 4, 8, 32, 64, 128]
    assert [s7.phase_tiles(l["decimation"], 16) for l in lv] == [4, 8, 16, 64, 128, 256]
    assert [l["nblk"] for l in lv if l["decimation"] >= 2048] == [1, 1]
    assert all(16 <= l["halo"] <= 48 for l in lv)
    # R = 4096 is the largest decimation an FFT of 2^20 points allows: M = P / R = 256, one block's length
    assert max(l["decimation"] for l in lv) == 4096 and (1 << 20) // 4096 == s7.B
    # the two-tile level of the 16-column build is case C's R = 32
    assert any(s7.phase_tiles(l["decimation"], 16) == 2 for n, l in _family("A", plan_of))


def test_case_h_reaches_every_lane_class(plan_of):
    classes = {}
    for halo in s7.H_FREQS:
        for output in ("complex", "amplitude"):
            lv = [l for l in s7.levels(plan_of("H%d" % halo, output)) if l["decimation"] == 16]
            assert [l["halo"] for l in lv] == [halo] and lv[0]["kernel"] == "k_synth7" and lv[0]["nblk"] == 1
        classes[halo] = s7.lane_classes(halo)
    assert classes[16] == dict(keep1=16, keep14=16, keep2=16, keep13=16)
    assert classes[17] == dict(keep1=15, keep14=15, keep2=16, keep13=16)
    assert classes[31] == dict(keep1=1, keep14=1, keep2=16, keep13=16)
    assert classes[32] == dict(keep1=0, keep14=0, keep2=16, keep13=16)
    assert classes[33] == dict(keep1=0, keep14=0, keep2=15, keep13=15)
    assert classes[47] == dict(keep1=0, keep14=0, keep2=1, keep13=1)
    assert classes[48] == dict(keep1=0, keep14=0, keep2=0, keep13=0)
    hw = s7.levels(plan_of("HW"))
    assert [(l["halo"], l["kernel"]) for l in hw] == [(46, "k_synth7"), (66, "k_synth7w"), (41, "k_synth7")]
    assert all(l["band_shift"] > 0 for l in hw)
    # without option interp = 0 the amplitude plan sends R = 16 to the interpolating kernel
    assert s7.make_plan("H32", "amplitude").info["n_interp"] == 1


def test_case_s_is_one_batch_of_two_segments(plan_of):
    for name in ("S", "Sa"):
        plan = plan_of(name, s7.CASES[name]["outputs"][0])
        (a0, a1), (b0, b1) = s7.S_EPOCHS
        # odd bounds; the gap between two odd bounds is even: a multiple of neither 4 nor 64
        assert all(v % 2 and v % 64 for v in (a0, a1, b0, b1)) and (b0 - a1) % 4 and (b0 - a1) % 64
        assert plan.segments() == [(a0, a1, 1 << 14), (b0, b1, 1 << 14)] and plan.debug_batches() == [(0, 2)]
        assert [int(s - (s & ~63)) for s in (a0, b0)] == [3, 55]
        assert plan.n_channels == 3
        # the second segment is the shorter one: on the batch's grid its last groups of blocks keep nothing of it and
        # leave at once, in both column builds and with R = 2 in either (synth7_narrow_r); none of the first's do
        for cols, narrow_r in ((32, 2), (32, 0), (32, 4), (16, 0)):
            gone = s7.early_groups(plan, cols, narrow_r)
            for r in (2, 4, 8) + ((16,) if name == "S" else ()):
                (g0, g1), groups = gone[r]
                assert g0 == 0 and 0 < g1 < groups, (name, cols, narrow_r, r, gone[r])
        assert s7.early_groups(plan, 32)[2] == ([0, 2], 5) and s7.early_groups(plan, 16)[8] == ([0, 2], 5)
        # the grid is the batch's: the second segment on its own would need fewer blocks at every level up to R = 16
        own = [-(-(-(-(55 + b1 - b0) // lv["decimation"])) // lv["hop"]) for lv in plan.debug_levels(1)]
        grid = [lv["nblk"] for lv in plan.debug_levels(1)]
        assert grid == [lv["nblk"] for lv in plan.debug_levels(0)]
        assert all(o < g for o, g, lv in zip(own, grid, plan.debug_levels(1)) if lv["decimation"] <= 16), (own, grid)
        assert s7.table(plan)[:3] == s7.EXPECT["Sa"]


@pytest.mark.parametrize("name", list(s7.CASES))
def test_stage_model_is_the_whole_path_model_and_meets_the_oracle(plan_of, name):
    """The stage model from the float64 ``level_input`` against ``cwt_decimated`` / ``morlet_model.cwt_decimated`` (the
    same quantity block by block with explicit polyphase twiddles) at float64 noise, and against the oracle within
    MODEL_CPU (MORLET_CPU for Morlet plans); every k_synth7 row, every sample."""
    c, plan = s7.CASES[name], plan_of(name)
    rows = _k7_rows(plan)
    got = s7.stage_model(name, plan, s7.host_levels(name, plan))
    x = s7.signal(name)
    if c["w0"] is not None:
        ref = np.zeros_like(got)
        ref[rows] = morlet_model.cwt_decimated(x, c["fs"], c["f"], c["w0"], s7.epochs_of(name), plan=plan, rows=rows)
    else:
        ref = cwt_decimated(x, c["fs"], c["f"], s7.epochs_of(name), c["gamma"], c["beta"], plan=plan, rows=set(rows.tolist()))
    noise = MODEL_NOISE_SHIFTED if any(lv["band_shift"] for lv in s7.levels(plan)) else MODEL_NOISE
    e_ref, e_or = rel_err(got[rows], ref[rows]), rel_err(got[rows], s7.oracle(name)[rows])
    print("%s: stage model against the whole-path model %.3g, against the oracle %.3g" % (name, e_ref.max(), e_or.max()))
    assert e_ref.max() < noise, e_ref
    assert e_or.max() < (MORLET_CPU if c["w0"] is not None else s7.MODEL_CPU), e_or


def test_what_the_stage_comparison_catches(plan_of):
    """Mutations of the model that stand for a kernel gone wrong, against the unmutated model on case A1's R = 4 level
    (16 scales, the ramp at 8): each must exceed the cap on the stage bound tenfold on the rows it touches.  A first
    layer cut one input too short (j_hi - 1) is printed, not asserted: it removes bins that are only just above the
    2e-7 the planner prunes by."""
    from decimated_model import synth_stage
    name = "A1"
    plan, c = plan_of(name), s7.CASES[name]
    lv = [l for l in s7.levels(plan) if l["decimation"] == 4][0]
    xr = s7.host_levels(name, plan)(0, lv["level"])
    rows = [int(i) for i in lv["rows"]]
    H = [s7.response(name, plan, i, lv) for i in rows]

    def row(h):
        return synth_stage(xr, h, 0, 4, lv["halo"], lv["hop"], 0, c["n"])
    ref = [row(h) for h in H]
    err = lambda y, r: np.abs(y - r).max() / np.abs(r).max()
    k = np.arange(256)
    ramp = np.exp(-1j * np.pi * k / (256 * 4))
    e = lv["n_plain"]                                      # the first scale of even length
    caught = {
        "ramp left out": err(row(H[e] / ramp), ref[e]),
        "ramp on the scale before": err(row(H[e - 1] * ramp), ref[e - 1]),
        "gains of the previous chunk": err(row(H[e - 8]), ref[e]),
        "one bin of the gain row lost": err(row(np.where(k == int(np.argmax(np.abs(H[3]))), 0, H[3])), ref[3]),
        "one kept sample not stored": err(np.where(np.arange(c["n"]) == 12345, 0, ref[5]), ref[5]),
    }
    for what, v in caught.items():
        print("%s: %.3g" % (what, v))
        assert v > 10 * s7.STAGE_CAP, what
    short = []
    for i, h, r, j_hi in zip(rows, H, ref, s7.predicted_j_hi(name, plan, lv)):
        short.append(err(row(np.where(k >= 16 * (j_hi - 1), 0, h)), r))
    print("first layer one input too short: %.3g .. %.3g, %d of %d rows over the cap" % (
        min(short), max(short), sum(v > s7.STAGE_CAP for v in short), len(short)))


@pytest.mark.parametrize("narrow_r", (0, 2))
@pytest.mark.parametrize("cols", (16, 32))
@pytest.mark.parametrize("name", list(s7.CASES))
def test_restated_groups_are_the_librarys_items(plan_of, option, name, cols, narrow_r):
    """``block_groups`` x ``phase_tiles`` against the items the library cuts (``debug_work_items``: what the upload
    sends), per level and per list -- the 16-column list of the levels up to synth7_narrow_r in a 32-column plan, the
    wide-halo list (halo > 48), the plain one -- and every item's first block a multiple of the blocks per group."""
    option("synth_cols", cols)
    option("synth7_narrow_r", narrow_r)
    output = s7.CASES[name]["outputs"][0]
    plan = plan_of(name, output)
    got = {k: plan.debug_work_items(k)["items"] for k in ("synth7", "synth7_wide", "synth7_narrow")}
    total = 0
    for lv in s7.levels(plan):
        on7 = lv["kernel"].startswith("k_synth7")
        narrow = cols == 32 and lv["decimation"] <= narrow_r and lv["halo"] <= 48
        mine = "synth7_wide" if lv["halo"] > 48 else "synth7_narrow" if narrow else "synth7"
        c = 16 if narrow else cols
        want = s7.block_groups(lv, c)[0] * s7.phase_tiles(lv["decimation"], c) if on7 else 0
        for k, items in got.items():
            its = items[items["level"] == lv["level"]]
            assert its.size == (want if k == mine else 0), (name, lv["decimation"], k)
            assert not (its["blk0"] % max(1, c // lv["decimation"])).any()
            assert not its.size or sorted(set(its["rtile"].tolist())) == list(range(s7.phase_tiles(lv["decimation"], c)))
        total += want
    assert total == sum(items.size for items in got.values()) and total > 0
