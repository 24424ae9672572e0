"""The cases of the full-band, block-convolution and time-domain paths without a device (tests/exact_cases.py): the
planner puts every case on the row of the table it is listed for, option bc_chunk_blocks changes the workspace and
nothing else, the float64 models of the three paths meet the oracle, the single-precision references the tighter gates
are taken from stay inside the project's gate on every case's recording, and the comparison catches nine kinds of
damage done to a model's own output at ten times a gate or more.  A planner change that moves a case off its branch
fails here, not silently in tests/test_gpu_exact_matrix.py."""
import numpy as np
import pytest

import exact_cases as ec
import level_cases as lc

QUARTER = ec.TOL / 4


def _offset_channel(name):
    return 1 if ec.CASES[name]["channels"] > 1 else 0


@pytest.mark.parametrize("name", list(ec.EXPECT))
def test_every_case_plans_onto_its_row(name):
    c, e = ec.CASES[name], ec.EXPECT[name]
    plan = ec.make_plan(name)
    si = plan.scale_info()
    assert si["method"].tolist() == e["methods"]
    assert si["length"].tolist() == e["lengths"] == [length for _, length in ec.kernels(name)]
    assert [(g["hop"], g["back"], g["scales"]) for g in plan.debug_blockconv()][:len(e["groups"])] == e["groups"]
    assert plan.info["n_blockconv"] == sum(len(g[2]) for g in e["groups"])
    if e["p"] is not None:
        assert {s[2] for s in plan.segments()} == {e["p"]} and e["p"] == e["p1"] * ec.ROW
        assert plan.debug_batches() == e["batches"]
    if name != "F4x":
        assert ec.whole_epochs(name, plan)
    for prec in c["precisions"][1:]:
        if prec != "exact":
            assert ec.make_plan(name, prec).scale_info()["method"].tolist() == e["methods"]


def test_full_band_cases_reach_their_branches():
    # F1: two segments of P1 = 1 in one batch, leads 7 and 3
    assert [s[0] & 63 for s in ec.make_plan("F1").segments()] == [7, 3]
    # F4 and F64: nine full-band scales are sets of 4 + 4 + 1 (kernels.h: kFullbandSet); the subsets give 1, 2, 3
    assert len(ec.F9) == 9 and sorted(len(s) for s in ec.F4_SUBSETS) == [1, 2, 3]
    for sub in ec.F4_SUBSETS:
        assert ec.make_plan("F4", scales=sub).scale_info()["method"].tolist() == [2] * len(sub)
    # F64, F128: the row pass's default group (32) is below P1, so bid / per > 0; per = group x slots
    for name, slots in (("F64", 4), ("F128", 3)):
        e, c = ec.EXPECT[name], ec.CASES[name]
        assert e["p1"] > 32 and c["channels"] * e["batches"][0][1] == slots
        for g in ec.GROUP_CASES[name]:
            assert (e["p1"] % g == 0) == (g != 3)                    # 3 falls back to the default
    assert 32 * 3 == 96
    # F8 under precision = exact: the 491-tap scale by blocks (with a ramp), the other full band
    p = ec.make_plan("F8", "exact")
    assert p.scale_info()["method"].tolist() == [ec.METHOD_BLOCKCONV, ec.METHOD_FULLBAND]
    assert [(g["hop"], g["back"], g["scales"]) for g in p.debug_blockconv()] == [(3072, 512, [0])]
    assert ec.make_plan("F8", "fast").scale_info()["method"].tolist() == [2, 2]
    # F4x: 22 time blocks of 2^14 points; 16 x 36 = 576 slots split the set of four over 3 workgroups, so that one
    # of them makes two scales (launch_fullband4: min(n, 2048 / slots)); the last batch's 216 slots split it over 4
    c = ec.CASES["F4x"]
    p = ec.make_plan("F4x")
    assert len(p.segments()) == 22 and p.debug_batches() == [(0, 16), (16, 6)]
    assert 2048 // (c["channels"] * 16) == 3 < 4 <= 2048 // (c["channels"] * 6)
    assert not ec.whole_epochs("F4x", p)


def test_block_cases_reach_their_edges():
    eb = ec.epochs_of("B1")
    hop, back = ec.EXPECT["B1"]["groups"][0][:2]
    assert eb[0, 0] % hop != 0                                        # starts mid-block
    assert eb[1, 1] - eb[1, 0] < hop                                  # shorter than a block
    assert eb[2, 0] == 7 * hop and eb[2, 1] - eb[2, 0] < back         # on an odd block, shorter than `back`
    assert eb[3, 1] == eb[4, 0] == 12 * hop                           # two epochs touch on a block edge
    # the smallest hop: kernels of 2400 .. 2559 taps
    assert ec.EXPECT["B1"]["groups"][1][:2] == (1536, 1280) and 2400 <= ec.EXPECT["B1"]["lengths"][-1] <= 2559
    lengths = ec.EXPECT["B1"]["lengths"]
    for _, _, scales in ec.EXPECT["B1"]["groups"]:
        assert {lengths[i] % 2 for i in scales} == {0, 1}            # odd and even lengths in both groups
    # precision = exact: no time domain, kernels beyond 1024 taps full band, one group with a ramp
    p = ec.make_plan("B1", "exact")
    assert p.scale_info()["method"].tolist() == [3] * 6 + [2] * 3
    assert [(g["hop"], g["back"]) for g in p.debug_blockconv()] == [(2944, 576)]
    # B2: 17 epochs, two flushes; lengths from 9 samples to more than a block
    e2 = ec.epochs_of("B2")
    assert len(e2) == ec.SEG_BATCH + 1 and (e2[:, 1] - e2[:, 0]).min() == 9 and (e2[:, 1] - e2[:, 0]).max() == 6000
    assert e2[-1, 1] <= ec.CASES["B2"]["n"] and np.all(e2[1:, 0] >= e2[:-1, 1]) and np.any(e2[1:, 0] == e2[:-1, 1])
    # B3: chunks of 2 and 6 blocks put seams inside an epoch and between epochs, in both groups
    for hop, _, _ in ec.EXPECT["B1"]["groups"]:
        for chunk in ec.CHUNKS:
            seams = ec.launch_chunks(eb, hop, chunk)
            assert any(k > 0 for _, k in seams) and any(k == 0 for _, k in seams), (hop, chunk)
    # execute_block ranges inside the recording
    for a, ln in ec.B1_RANGES:
        assert 0 <= a and a + ln <= ec.CASES["B1"]["n"]


def test_time_domain_cases_reach_their_edges():
    for name in ec.DIRECT_CASES:
        si = ec.make_plan(name).scale_info()
        assert set(si["method"].tolist()) == {ec.METHOD_DIRECT}, name
    si = ec.make_plan("D1s").scale_info()
    assert len({int((L - 1) // 2) % 8 for L in si["length"]}) == 8 and 33 <= si["length"].min() and si["length"].max() <= 48
    assert ec.make_plan("D1l").scale_info()["length"].max() == 241
    e2, e3 = ec.epochs_of("D2"), ec.epochs_of("D3")
    assert e2[1, 1] - e2[1, 0] == 9
    assert len(e3) == ec.SEG_BATCH + 1 and e3[-1, 1] <= ec.CASES["D3"]["n"] and np.all(e3[1:, 0] > e3[:-1, 1])
    assert (e3[:, 1] - e3[:, 0]).min() == 9


def test_bc_chunk_blocks_caps_the_workspace_and_nothing_else():
    """Unset or 0: the plan's workspace as before; a value caps the blocks in hand at whole pairs, never below two, never
    above what the plan had; plans without block convolution do not see it."""
    base = ec.make_plan("B1")
    ws = base.info["workspace_bytes"]
    c = ec.CASES["B1"]["channels"]
    per_pair = 2 * 8 * ec.ROW * c
    assert ec.make_plan("B1", bc_chunk_blocks=0).info["workspace_bytes"] == ws
    assert ec.make_plan("B1", bc_chunk_blocks=1 << 40).info["workspace_bytes"] == ws
    w2, w6 = (ec.make_plan("B1", bc_chunk_blocks=k).info["workspace_bytes"] for k in ec.CHUNKS)
    assert w6 - w2 == 2 * per_pair and w2 < w6 < ws
    # unset, the plan holds what it always held: n / (smallest hop) + 2 per epoch + 1 blocks, + 2, in whole pairs
    blocks = (ec.CASES["B1"]["n"] // 1536 + 2 * len(ec.epochs_of("B1")) + 1 + 2) & ~1
    assert blocks == 52 and ws - w2 == (blocks - 2) // 2 * per_pair
    assert ec.make_plan("B1", bc_chunk_blocks=1).info["workspace_bytes"] == w2
    assert ec.make_plan("B1", bc_chunk_blocks=3).info["workspace_bytes"] == w2
    assert ec.make_plan("B1", bc_chunk_blocks=7).info["workspace_bytes"] == w6
    assert ec.make_plan("B1", bc_chunk_blocks=-5).info["workspace_bytes"] == ws
    for k in (2, 6):
        q = ec.make_plan("B1", bc_chunk_blocks=k)
        assert q.scale_info()["method"].tolist() == base.scale_info()["method"].tolist()
        assert q.debug_blockconv() == base.debug_blockconv()
    assert ec.make_plan("F4", bc_chunk_blocks=2).info["workspace_bytes"] == ec.make_plan("F4").info["workspace_bytes"]


def test_recordings_tell_channels_apart():
    for name, c in ec.CASES.items():
        x = ec.recording(name)
        assert x.dtype == np.float32 and x.shape == (c["channels"], c["n"])
        assert len({row.tobytes() for row in x}) == c["channels"]
        if c["channels"] > 1:
            assert abs(float(x[1].mean()) - ec.OFFSET) < 1.0 and abs(float(x[0].mean())) < 1.0
    np.testing.assert_array_equal(ec.recording("B4-1")[0], ec.recording("B4-5")[0])


def test_response_from_the_library_is_the_numpy_one():
    """Beyond 2^15 points H comes from the library's host evaluation of the closed form: the same numbers as
    decimated_model.exact_gain, on bins spread over a 2^18-point grid."""
    plan = ec.make_plan("F64")
    p = ec.EXPECT["F64"]["p"]
    k = np.unique(np.concatenate([np.arange(64), np.arange(p // 2 - 32, p // 2 + 32), np.arange(p - 64, p),
                                  np.random.default_rng(3).integers(0, p, 400)]))
    for i, (om, length) in enumerate(ec.kernels("F64")):
        mine = ec.exact_gain(2 * np.pi * k / p, om, length, 3.0, 2.0)
        theirs = plan.debug_exact_gain(i, k, p)
        assert np.abs(mine - theirs).max() <= 1e-12 * np.abs(mine).max(), i
        assert np.abs(ec.response("F64", i, p, plan)[k] - mine * np.exp(-2j * np.pi * k * (0.5 * ((length - 1) % 2)) / p)).max() \
            <= 1e-12 * np.abs(mine).max()


@pytest.mark.parametrize("name", list(ec.CASES))
def test_models_meet_the_oracle_and_single_precision_stays_inside_the_gate(name):
    """Every precision of the case, every scale, the channel with the offset and channel 0: the float64 model of the path
    the plan takes is the oracle's row to a quarter of the gate (it is far closer), and the single-precision reference
    of that path stays inside the project's gate."""
    c = ec.CASES[name]
    channels = sorted({0, _offset_channel(name)}) if c["n"] <= 100000 else [_offset_channel(name)]
    worst = [0.0, 0.0]
    for prec in c["precisions"]:
        if prec == "fast":
            continue                                      # (the same methods, pinned above: the same models)
        plan = ec.make_plan(name, prec)
        for ch in channels:
            ref = ec.oracle(name, ch)
            for i in range(len(c["f"])):
                model = ec.row_model(name, plan, ch, i, False, prec == "exact")
                assert lc.compare(model, ref[i])[0] < QUARTER, (name, prec, ch, i)
                assert np.all(model[ec.outside(name)] == 0)
                mx, rms = lc.compare(ec.row_model(name, plan, ch, i, True, prec == "exact"), ref[i])
                worst = [max(worst[0], mx), max(worst[1], rms)]
                assert mx < ec.TOL, (name, prec, ch, i, mx)
    print("case %s: single precision max %.2e rms %.2e" % (name, *worst))


def _seg(name, plan, ch, seg=0):
    a, b, p = plan.segments()[seg]
    s_in = lc.segment_input(ec.recording(name)[ch], a, b)
    return lc.spectrum(s_in, p), lc.spectrum(s_in, p, single=True), a & 63, b - a, p


@pytest.mark.parametrize("name", ec.FULLBAND_CASES)
def test_full_band_mutations(name):
    """(i) the twiddle of spectrum row P1 - 1 one step on in the inverse, (ii) two slots exchanged (F128), (iii) the crop
    one sample late, (iv) rows n1 = 1 and 3 of the 4-row DFT exchanged (F4), (v) a neighbouring scale's response used
    inside a set: each misses a gate by CAUGHT or more, on the first and the last full-band scale."""
    plan = ec.make_plan(name)
    p1 = ec.EXPECT[name]["p1"]
    X, X32, lead, ne, p = _seg(name, plan, 0, seg=len(plan.segments()) - 1)
    full = np.flatnonzero(plan.scale_info()["method"] == ec.METHOD_FULLBAND)
    for i in (full[0], full[-1]):
        h = ec.response(name, i, p, plan)
        ref = ec.fullband_row(X, h, lead, ne)
        single = ec.fullband_row(X32, h, lead, ne, single=True)
        assert lc.compare(single, ref)[0] < ec.TOL
        if p1 > 1:
            f = ec.factor(ec.fullband_row_twiddle_late(X, h, lead, ne, p1), ref, ec.TOL, single)
            print("%s scale %d (i) twiddle of row %d one step on: %.1f x" % (name, i, p1 - 1, f))
            assert f >= lc.CAUGHT, (name, i, f)
        if name == "F128":
            other = _seg(name, plan, 2)[0]
            f = ec.factor(ec.fullband_row(other, h, lead, ne), ref, ec.TOL, single)
            print("%s scale %d (ii) slot 2 for slot 0: %.3g x" % (name, i, f))
            assert f >= lc.CAUGHT
        f = ec.factor(ec.fullband_row(X, h, lead, ne, crop_late=1), ref, ec.TOL, single)
        print("%s scale %d (iii) crop one sample late: %.3g x" % (name, i, f))
        assert f >= lc.CAUGHT
        if name == "F4":
            f = ec.factor(ec.fullband_row_dft4_swapped(X, h, lead, ne), ref, ec.TOL, single)
            print("%s scale %d (iv) rows 1 and 3 of the DFT4 exchanged: %.3g x" % (name, i, f))
            assert f >= lc.CAUGHT
        if full.size > 1:
            j = full[1] if i == full[0] else full[-2]
            f = ec.factor(ec.fullband_row(X, ec.response(name, j, p, plan), lead, ne), ref, ec.TOL, single)
            print("%s scale %d (v) the response of scale %d: %.3g x" % (name, i, j, f))
            assert f >= lc.CAUGHT


def test_block_convolution_mutations():
    """B1, both groups, the shortest and the longest kernel of each: (vi) one block's hop taken one sample late, (vii) the
    two blocks of a pair exchanged, (viii) the block on a chunk seam left zero -- each seam of bc_chunk_blocks = 2 and 6
    that falls on a block with output, one at a time."""
    name = "B1"
    plan = ec.make_plan(name)
    x = ec.recording(name)[0].astype(np.float64)
    xm = x - x.mean()
    eb = ec.epochs_of(name)
    for g in plan.debug_blockconv():
        hop, back = g["hop"], g["back"]
        for i in (g["scales"][0], g["scales"][-1]):
            h = ec.bc_response(name, i)
            ref = ec.bc_row(xm, eb, hop, back, h)
            single = ec.bc_row(xm, eb, hop, back, h, single=True)
            assert lc.compare(single, ref)[0] < ec.TOL
            for where in ((0, 2), (4, 1)):                                                       # (epoch, block of it)
                f = ec.factor(ec.bc_row(xm, eb, hop, back, h, late_block=where), ref, ec.TOL, single)
                print("hop %d scale %d (vi) block %s one sample late: %.3g x" % (hop, i, where, f))
                assert f >= lc.CAUGHT
                f = ec.factor(ec.bc_row(xm, eb, hop, back, h, swap_pair=where), ref, ec.TOL, single)
                print("hop %d scale %d (vii) blocks %s and the next exchanged: %.3g x" % (hop, i, where, f))
                assert f >= lc.CAUGHT
            seen, least = 0, np.inf
            for chunk in ec.CHUNKS:
                for ei, k in ec.launch_chunks(eb, hop, chunk):
                    q = int(ec.bc_blocks(*eb[ei], hop)[k])
                    if max(q * hop, eb[ei, 0]) >= min((q + 1) * hop, eb[ei, 1]):
                        continue                                  # a block that only completes a pair: no output
                    f = ec.factor(ec.bc_row(xm, eb, hop, back, h, zero_block=(ei, k)), ref, ec.TOL, single)
                    assert f >= lc.CAUGHT, (hop, i, chunk, ei, k, f)
                    seen, least = seen + 1, min(least, f)
            print("hop %d scale %d (viii) %d seam blocks left zero, one at a time: %.3g x or more" % (hop, i, seen, least))
            assert seen >= 8


@pytest.mark.parametrize("name", ec.DIRECT_CASES)
def test_time_domain_mutations(name):
    """(ix) k_direct's sum without Psi[L - 1] x~[q - L + 1].  FINDING: no comparison can catch this one.  Psi[L - 1] is
    the sum of the kernel's taps, the kernel is the inverse DFT of L spectrum samples A_j (morseutils.py:147-149) and A_0
    is the wavelet at zero frequency, which is zero: the taps sum to 1e-16 of their largest for every kernel the
    reference builds, the term is far below half an ulp of any output, and dropping it changes nothing (asserted: under
    1e-6 of a gate).  What carries the weight of the summation by parts at an epoch's edge is the difference behind its
    last sample, d[Ne] = -x~[Ne - 1]: (ix') that difference dropped misses a gate by CAUGHT or more on every kernel."""
    c = ec.CASES[name]
    x32 = ec.recording(name)[0]
    mean = float(x32.astype(np.float64).mean())
    eb = ec.epochs_of(name)
    args = (x32, mean, eb)
    for om, length in ec.kernels(name):
        kw = (om, length, c["gamma"], c["beta"])
        ref = ec.direct_row(*args, *kw, single=False)
        single = ec.direct_row(*args, *kw, single=True)
        f_tail = ec.factor(ec.direct_row(*args, *kw, single=False, drop_tail=True), ref, ec.TOL, single)
        f_end = ec.factor(ec.direct_row(*args, *kw, single=False, drop_end=True), ref, ec.TOL, single)
        plain = ec.plain_float32_row(*args, *kw)
        print("%s L %d (ix) tail term dropped: %.3g x; (ix') last difference dropped: %.3g x; a plain float32 convolution has"
              " %.2f x the rms error of the kernel's order" % (name, length, f_tail, f_end,
                                                               lc.compare(plain, ref)[1] / lc.compare(single, ref)[1]))
        assert f_tail < 1e-6, (name, length, f_tail)
        assert f_end >= lc.CAUGHT, (name, length, f_end)
