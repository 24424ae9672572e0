"""k_synth7 (csrc/synth.hip, synth_morlet.hip) against the float64 model of its own stage, from its own input, at every
chunk, ramp, window, phase-tile, halo and segment edge: the cases of tests/synth7_cases.py (pinned on the host by
tests/test_synth7_cases_cpu.py) on the device.  Every k_synth7 row goes against the stage model -- steps 3 and 4 of
DESIGN.md section 3 in float64 from the x_R the device itself holds, with the exact gains -- and every row against the
oracle, over every sample; whole executes write into a buffer of NaNs with a padded pitch and must leave nothing
unwritten and nothing beside the rows touched; the instantiations (column builds, item orders, channel counts) and
block requests must reproduce the default plan's rows to the bit.  Figures and how the bounds were set:
profiles/synth7_matrix.md."""
import numpy as np
import pytest
from scipy.fft import fft

import synth7_cases as s7
from conftest import rel_err

pytestmark = pytest.mark.gpu

# Worst row of each family against the stage model, measured on an MI355X (profiles/synth7_matrix.md), complex /
# amplitude / power (power rows against |model|^2 on the same metric: about twice the amplitude's figure,
# |y^2 - r^2| = 2 e max|r|^2 for |y - r| = e max|r|):
#   A    4.70e-7 / 4.96e-7 / 8.29e-7      A256 4.94e-7 / 4.91e-7      M    6.19e-7 / 5.65e-7 (w0 = 4, shifted bands)
#   W    4.74e-7 (5.08e-7 with fuse_blocks = 0)      H    3.93e-7 / 4.02e-7      S    4.85e-7 / 4.54e-7
# Three times the worst of them is 2.5e-6, above the cap, so the cap is the bound -- for power rows as for the others.
# Why the kernel reads 1.5 to 2 x what a float32 emulation with pocketfft does (1.6e-7 .. 3.2e-7) is accounted for in
# profiles/synth7_matrix.md: the polyphase twiddles as a running product of sixteen float32 steps, table twiddles in
# four DFT16 passes, and for the shifted Morlet levels two carriers and a complex gain more.
STAGE_WORST = 8.29e-7
STAGE_BOUND = min(3 * STAGE_WORST, s7.STAGE_CAP)   # (the cap: the whole path shows 6.2e-7 for these rows, forward stages included)
GATE_BLOCKS = 3e-6              # block spectra against the transform of the device's x_R (tests/test_gpu_stages.py)
# float32 |complex row| (hypot in float64, rounded once) against the amplitude row, its square against the power row,
# in last places.  Both modes make the same z (the mode only picks the store); amplitude: z.x^2 rounded, the fused
# z.y^2 + . rounded (1 ulp of p2 together, half of it left after the root), v_sqrt_f32 1 ulp, one rounding of the
# reference (1/2); power: 1 ulp of p2 and the reference's 1/2.  Worst measured: 1 in both modes, every case of A and H
# -> twice it.
ULP_WORST = {"amplitude": 1, "power": 1}
ULP_BOUND = {k: 2 * v for k, v in ULP_WORST.items()}

FILL, PAD = 0x7FC12345, 0x7FC0BEEF        # NaN bit patterns: every float of a row, every float of the pad behind it
_ROWS, _XR, _MODEL = {}, {}, {}


def _set(option, name, output, extra=None):
    opts = dict(s7.plan_options(name, output))
    opts.update(extra or {})
    for k, v in opts.items():
        option(k, v)
    return opts


def _clear(option, opts):
    for k in opts:
        option(k, None)


def _recordings(name, n_channels, tiled=False):
    return np.stack([s7.signal(name, 0 if tiled else ch) for ch in range(n_channels)])


def _outside(name):
    m = np.ones(s7.CASES[name]["n"], bool)
    for a, b in s7.epochs_of(name):
        m[a:b] = False
    return m


def _fetch_levels(name, plan):
    """{(channel, epoch, level): x_R over the FFT length, complex128} of every k_synth7 level after an execute."""
    segs = plan.segments()
    out = {}
    for lv in s7.levels(plan):
        if lv["kernel"].startswith("k_synth7"):
            for e in range(len(segs)):
                for ch in range(plan.n_channels):
                    out[(ch, e, lv["level"])] = plan.debug_fetch(1, ch, e, lv["level"]).astype(np.complex128) / segs[e][2]
    return out


def _into_nans(name, plan, x):
    """Whole execute, device in and device out, into a buffer whose every float is a NaN and whose rows are padded
    (the pad holds another NaN): every sample inside an epoch is written (finite), every sample outside is exactly
    zero, the pad is untouched; the same again into the same buffer, re-filled: bit-equal.  Returns rows (C, S, n)."""
    from ghost_amd.engine import DeviceBuffer
    c = s7.CASES[name]
    n, S, C = c["n"], len(c["f"]), plan.n_channels
    elem = 2 if plan.out_dtype == np.complex64 else 1
    pitch = ((n + 31) & ~31) + 32
    fill = np.full((C * S, pitch * elem), PAD, np.uint32)
    fill[:, :n * elem] = FILL
    xb, ob = DeviceBuffer(x.nbytes), DeviceBuffer(fill.nbytes)
    try:
        xb.upload(np.ascontiguousarray(x, dtype=np.float32))
        plan.set_row_pitch(pitch)
        runs = []
        for _ in range(2):
            ob.upload(fill)
            plan.execute_device(xb, ob)
            runs.append(ob.download(fill.shape, np.uint32))
    finally:
        plan.set_row_pitch(0)
        xb.free()
        ob.free()
    first, again = runs
    assert np.all(first[:, n * elem:] == PAD), "%s: the pad behind the rows was written" % name
    vals = first[:, :n * elem].view(np.float32).reshape(C * S, n, elem)
    inside = ~_outside(name)
    assert np.isfinite(vals[:, inside]).all(), "%s: %d floats inside the epochs were left unwritten" % (
        name, int((~np.isfinite(vals[:, inside])).sum()))
    assert not first[:, :n * elem].reshape(C * S, n, elem)[:, ~inside].any(), "%s: not zero outside the epochs" % name
    np.testing.assert_array_equal(again, first, err_msg="%s: a second execute into the same buffer" % name)
    rows = np.ascontiguousarray(first[:, :n * elem]).view(plan.out_dtype).reshape(C, S, n)
    return rows


def _run(option, name, output, extra=None, n_channels=None, tiled=False, nans=True):
    """(plan, rows (C, S, n)) of a whole execute under the case's options and `extra`."""
    opts = _set(option, name, output, extra)
    plan = s7.make_plan(name, output, n_channels)
    _clear(option, opts)
    x = _recordings(name, plan.n_channels, tiled)
    rows = _into_nans(name, plan, x) if nans else plan.execute(x)
    assert plan.precision_report()["rerouted"] == 0          # the rows are the decimated path's, not the exact one's
    assert plan.info["n_interp"] == 0
    return plan, rows


def whole(option, name, output):
    """The default plan's rows of a case (C, S, n), made once through ``_into_nans`` and read-only, with the x_R of
    every k_synth7 level as the device held it."""
    key = (name, output)
    if key not in _ROWS:
        plan, rows = _run(option, name, output)
        # the branches the case is there for, reached by the plan that made the rows (test_synth7_cases_cpu.py reads
        # chunk sizes, ramp positions, phase tiles, lane classes and block counts off this table)
        assert s7.table(plan) == s7.EXPECT[name], (name, output)
        assert plan.debug_batches() == [(0, len(s7.epochs_of(name)))]
        assert all(9 <= j <= 16 for lv in s7.levels(plan) for j in lv["j_hi"])
        rows.setflags(write=False)
        _ROWS[key], _XR[key] = rows, _fetch_levels(name, plan)
        plan.close()
    return _ROWS[key]


def model(option, name, output, channel=0):
    """complex128 (S, n): the stage model of one channel from the x_R the default plan of (name, output) left on the
    device.  Made once per case and channel: another output mode whose x_R has the same bits reuses it."""
    whole(option, name, output)
    plan = s7.make_plan(name, "complex")          # (planning only: the levels are the same in every mode, pinned on the host)
    xr = {k[1:]: v for k, v in _XR[(name, output)].items() if k[0] == channel}
    for got_xr, got in _MODEL.get((name, channel), []):
        if all(np.array_equal(xr[k], got_xr[k]) for k in xr):
            plan.close()
            return got
    got = s7.stage_model(name, plan, lambda e, level: xr[(e, level)])
    plan.close()
    got.setflags(write=False)
    _MODEL.setdefault((name, channel), []).append((xr, got))
    return got


_K7 = {}


def _k7_rows(name):
    if name not in _K7:
        plan = s7.make_plan(name, "complex")
        _K7[name] = np.sort(np.concatenate([lv["rows"] for lv in s7.levels(plan) if lv["kernel"].startswith("k_synth7")]))
        plan.close()
    return _K7[name]


def _stage_error(output, got, mod):
    """Per row against the model in the row's mode (conftest.rel_err): |model|, |model|^2 for power rows."""
    return rel_err(got, s7.as_output(output, mod))


RUNS = [(name, output) for name, c in s7.CASES.items() for output in c["outputs"]]


@pytest.mark.parametrize("name, output", RUNS)
def test_rows_against_stage_model_and_oracle(option, name, output):
    """(a), (b), (c): every k_synth7 row of every channel within STAGE_BOUND of the stage model made from that channel's
    own x_R, every row within the gate of the oracle, every sample; the execute went into NaNs (``_into_nans``).  The
    branches the case is there for are asserted reached through the plan's hooks first."""
    got = whole(option, name, output)
    rows = _k7_rows(name)
    gate = 2 * s7.GATE if output == "power" else s7.GATE
    for ch in range(got.shape[0]):
        e_mod = _stage_error(output, got[ch][rows], model(option, name, output, ch)[rows])
        e_or = rel_err(got[ch], s7.as_output(output, s7.oracle(name, ch)))
        print("%s %s channel %d: stage model worst %.3g median %.3g; oracle worst %.3g median %.3g (%d rows, %d on k_synth7)"
              % (name, output, ch, e_mod.max(), np.median(e_mod), e_or.max(), np.median(e_or), got.shape[1], rows.size))
        assert e_mod.max() < STAGE_BOUND, (name, output, ch, e_mod)
        assert e_or.max() < gate, (name, output, ch, e_or)


def test_first_layer_windows_reached(option):
    """Every j_hi from 9 to 16 on at least one scale of case A, in amplitude / power (A1, A2) and in complex mode
    (C1, C2), read from the device's lists after k_scale_windows ran; the float64 prediction beside it."""
    for names, output in ((("A1", "A2"), "amplitude"), (("C1", "C2"), "complex")):
        seen = set()
        for name in names:
            plan = s7.make_plan(name, output)
            assert not any(lv["j_hi"].any() for lv in s7.levels(plan))
            plan.upload()
            for lv in s7.levels(plan):
                assert lv["j_hi"].min() >= 9 and lv["j_hi"].max() <= 16
                pred = s7.predicted_j_hi(name, plan, lv)
                print("%s R = %d: j_hi %s, differs from the float64 prediction on %d entries"
                      % (name, lv["decimation"], lv["j_hi"].tolist(), int((pred != lv["j_hi"]).sum())))
                assert np.abs(pred - lv["j_hi"]).max() <= 1
                seen |= set(lv["j_hi"].tolist())
            plan.close()
        assert seen == set(range(9, 17)), (output, seen)


D_CASES = [("A1", "complex"), ("A1", "amplitude"), ("A2", "power"), ("C2", "complex"), ("M4", "complex"),
           ("M6", "amplitude"), ("W", "complex"), ("H33", "amplitude"), ("HW", "complex"), ("S", "complex"),
           ("Sa", "amplitude")]


@pytest.mark.parametrize("name, output", D_CASES)
def test_instantiations_leave_the_bits_alone(option, name, output):
    """(d): 16 columns against 32 (the R = 2 .. 16 levels in workgroups of half as many blocks, R >= 32 in twice as many
    phase tiles), synth7_narrow_r = 0, 2, 4 (which levels take the 16-column build in a 32-column plan) and the three
    item orders: a column's arithmetic does not depend on which workgroup holds it, so the rows are bit-equal.  On case
    S the groups of blocks past the shorter segment's end leave at once, other groups in every build
    (synth7_cases.early_groups, pinned on the host)."""
    ref = whole(option, name, output)
    for extra in ({"synth_cols": 16}, {"synth_cols": 32}, {"synth7_narrow_r": 0}, {"synth7_narrow_r": 2},
                  {"synth7_narrow_r": 4}, {"synth7_order": 0}, {"synth7_order": 1}, {"synth7_order": 2},
                  {"synth_cols": 16, "synth7_order": 2}):
        plan, got = _run(option, name, output, extra, nans=False)
        np.testing.assert_array_equal(got, ref, err_msg="%s %s %s" % (name, output, extra))
        plan.close()


@pytest.mark.parametrize("name, output", [("A2", "complex"), ("A1", "amplitude")])
def test_channel_count_leaves_the_bits_alone(option, name, output):
    """(d): the same recording as 1, 3 and 33 channels."""
    ref = whole(option, name, output)[0]
    for c in (3, 33):
        plan, got = _run(option, name, output, n_channels=c, tiled=True, nans=False)
        for ch in range(c):
            np.testing.assert_array_equal(got[ch], ref, err_msg="%s %s, channel %d of %d" % (name, output, ch, c))
        plan.close()


@pytest.mark.parametrize("name, output", [("A1", "complex"), ("A1", "amplitude"), ("M4", "complex"), ("W", "complex"),
                                          ("HW", "complex")])
def test_separate_block_spectra_pass(option, name, output):
    """(d): fuse_blocks = 0 -- the block spectra come from the pass of their own, not from the kernel's prologue: rows
    within STAGE_BOUND of the stage model of that run's x_R, and the stored spectra (first and last block of every
    level) within GATE_BLOCKS of the transform of the device's x_R, as tests/test_gpu_stages.py has it."""
    plan, got = _run(option, name, output, {"fuse_blocks": 0})
    xr = {k[1:]: v for k, v in _fetch_levels(name, plan).items() if k[0] == 0}
    rows = _k7_rows(name)
    mod = s7.stage_model(name, plan, lambda e, level: xr[(e, level)])
    e_mod = _stage_error(output, got[0][rows], mod[rows])
    print("%s %s fuse_blocks = 0: stage model worst %.3g median %.3g" % (name, output, e_mod.max(), np.median(e_mod)))
    assert e_mod.max() < STAGE_BOUND, e_mod
    for lv in s7.levels(plan):
        if not lv["kernel"].startswith("k_synth7"):
            continue
        xb = plan.debug_fetch(2, level=lv["level"]).astype(np.complex128).reshape(lv["nblk"], 256)
        x_r = xr[(0, lv["level"])]
        for b in (0, lv["nblk"] - 1):
            ref_b = fft(x_r[(b * lv["hop"] - lv["halo"] + np.arange(256)) % x_r.size]) / 256.0
            assert np.abs(xb[b] - ref_b).max() < GATE_BLOCKS * np.abs(ref_b).max(), (name, lv["decimation"], b)
    plan.close()


def _check_windows(option, name, output, wins):
    ref = whole(option, name, output)
    opts = _set(option, name, output)
    plan = s7.make_plan(name, output)
    _clear(option, opts)
    x, n = _recordings(name, plan.n_channels), s7.CASES[name]["n"]
    for start, length in wins:
        assert 0 <= start and start + length <= n and length > 0, (start, length)
        got = plan.execute_block(x, start, length)
        np.testing.assert_array_equal(got, ref[..., start:start + length], err_msg="%s %s [%d, +%d)" % (name, output, start, length))
    plan.close()


def test_block_requests_on_phase_tiles(option):
    """(e), case W (R = 64 .. 4096, tiles of 32 phases; one block at R >= 2048): windows that start and end inside a
    phase tile at odd offsets -- inside one tile of every level, across tiles, across blocks --, one sample, the
    recording's two ends: bit-equal to the whole execute's columns."""
    n = s7.CASES["W"]["n"]
    wins = []
    for lv in s7.levels(s7.make_plan("W")):
        R, period = lv["decimation"], lv["hop"] * lv["decimation"]
        k = 1 if 2 * period < n else 0
        wins += [(k * period + 5 * R + 32 * 1 + 7, 19),                 # inside phase tile 1 of one decimated sample
                 (k * period + 5 * R + 32 * 1 + 7, 2 * R + 11),         # tiles of three decimated samples
                 (max(0, k * period - 33), 67)]                         # across a block edge (or the recording's start)
    wins += [(123457, 1), (4096 * 31 + 32 * 77 + 31, 1), (0, 777), (0, 1), (n - 1001, 1001), (n - 1, 1), (1, n - 2)]
    assert all(s % 2 == 1 or (s + l) % 2 == 1 for s, l in wins)
    _check_windows(option, "W", "complex", wins)


@pytest.mark.parametrize("output", ["complex", "amplitude"])
def test_block_requests_at_every_halo(option, output):
    """(e), the H cases (one block at R = 16, halo 16 .. 48) and the shifted levels of HW (halo 46 and 66)."""
    for name in [k for k in s7.CASES if s7.FAMILY[k] == "H"]:
        n = s7.CASES[name]["n"]
        wins = [(1, n - 2), (777, 1), (0, 333), (n - 333, 333), (37, 1001), (n - 1, 1)]
        _check_windows(option, name, output, wins)


@pytest.mark.parametrize("name, output", [("S", "complex"), ("Sa", "amplitude")])
def test_block_requests_across_the_gap(option, name, output):
    """(e), case S: windows that span the gap between the two segments, start in it, end in it, lie inside it."""
    (a0, a1), (b0, b1) = s7.S_EPOCHS
    n = s7.CASES[name]["n"]
    wins = [(a1 - 1001, 2003), (a1 - 1, 2), (a1, b0 - a1), (a1 + 1, 300), (a1 - 257, 258), (b0 - 1, 258), (0, 5),
            (b1 - 2, 6), (a1 - 3001, 6003), (a0, 1), (b1 - 1, 1), (b1, n - b1)]
    _check_windows(option, name, output, wins)


def _ulp_distance(a, b):
    """Last places between two non-negative float32 arrays."""
    assert a.dtype == b.dtype == np.float32 and (a >= 0).all() and (b >= 0).all()
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


F_CASES = [(n, o) for n, c in s7.CASES.items() if s7.FAMILY[n] in ("A", "H") for o in c["outputs"] if o != "complex"]


@pytest.mark.parametrize("name, output", F_CASES)
def test_output_modes_against_each_other(option, name, output):
    """(f): float32 |complex row| (hypot in float64, rounded once) against the amplitude row, its square (squared in
    float64, rounded once) against the power row, in last places; k_synth7 rows, every sample inside the epochs."""
    cx, other = whole(option, name, "complex")[0], whole(option, name, output)[0]
    rows = _k7_rows(name)
    re, im = cx[rows].real.astype(np.float64), cx[rows].imag.astype(np.float64)
    want = (np.hypot(re, im) if output == "amplitude" else re * re + im * im).astype(np.float32)
    ulp = _ulp_distance(want, other[rows])
    print("%s: |complex| against %s, worst %d ulp" % (name, output, ulp.max()))
    assert ulp.max() <= ULP_BOUND[output], (name, output, ulp.max())
