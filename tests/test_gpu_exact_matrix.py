"""The full-band, block-convolution and time-domain paths on the device (GPU), every case of tests/exact_cases.py:

1. the full band on its own input -- IFFT_P(X_dev H)[lead : lead + ne] in float64 from the spectrum fetched from the
   device, every row of every channel and segment, so that a failure names the inverse passes, the response or the
   crop and not the forward transform (tests/test_gpu_level_matrix.py holds that one);
2. every case end to end against the oracle's float64 convolution with the literal kernels, columns outside every epoch
   exactly zero;
3. bit equality wherever two plans execute the same arithmetic per row: fullband_group values, fullband_cache_mb = 0,
   a scale alone or in a smaller set, fullband4 = 0, bc_chunk_blocks, execute_block, a second execute.

Gates: the project's TOL = 1e-5 on conftest.rel_err (2 TOL on power rows), and rms(err) / rms(ref) at most four times
(level_cases.RMS_FACTOR) that of the path's single-precision reference computed here on the same data
(exact_cases.row_model).  profiles/exact_matrix.md has what was measured."""
import numpy as np
import pytest

import exact_cases as ec
import level_cases as lc
from conftest import rel_err

pytestmark = pytest.mark.gpu


def _tol(output):
    return 2 * ec.TOL if output == "power" else ec.TOL


def _gate(got, ref, single, hard, what, worst=None):
    """Both gates of one row."""
    mx, rms = lc.compare(got, ref)
    rms_ref = lc.compare(single, ref)[1]
    print("    %s: max %.3g rms %.3g (single precision %.3g: %.2f x)" % (what, mx, rms, rms_ref, rms / rms_ref))
    if worst is not None:
        worst[0], worst[1], worst[2] = max(worst[0], mx), max(worst[1], rms), max(worst[2], rms / rms_ref)
    assert mx < hard, (what, mx)
    assert float(rel_err(got, ref)) < hard, what
    assert rms <= lc.RMS_FACTOR * rms_ref, (what, rms, rms_ref)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _end_to_end(name, plan, got, prec, output, channels, worst):
    """Rows of ``channels`` against the oracle, with the single-precision reference of each row's own path."""
    c = ec.CASES[name]
    out = ec.outside(name)
    assert np.all(got[:, :, out] == 0)
    for ch in channels:
        ref = ec.oracle(name, ch)
        for i in range(len(c["f"])):
            single = ec.row_model(name, plan, ch, i, True, prec == "exact")
            _gate(got[ch, i], ec.as_output(ref[i], output), ec.as_output(single, output), _tol(output),
                  "%s channel %d scale %d end to end" % (output, ch, i), worst)


FULLBAND_RUNS = [(n, p) for n in ec.FULLBAND_CASES for p in ec.CASES[n]["precisions"]]


@pytest.mark.parametrize("name, prec", FULLBAND_RUNS, ids=["%s-%s" % r for r in FULLBAND_RUNS])
def test_full_band_on_its_own_input_and_end_to_end(name, prec):
    c = ec.CASES[name]
    x = ec.recording(name)
    plan = ec.make_plan(name, prec)
    result = plan.execute_resident(x)
    got = result.to_host()
    p1 = ec.EXPECT[name]["p1"]
    full = np.flatnonzero(plan.scale_info()["method"] == ec.METHOD_FULLBAND)
    own, end = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
    for seg, (a, b, p) in enumerate(plan.segments()):
        for ch in range(c["channels"]):
            X = lc.natural(plan.debug_fetch(0, channel=ch, epoch=seg).reshape(p1, ec.ROW).astype(np.complex128))
            for i in full:
                h = ec.response(name, int(i), p, plan)
                _gate(got[ch, i, a:b], ec.fullband_row(X, h, a & 63, b - a), ec.fullband_row(X, h, a & 63, b - a, single=True),
                      ec.TOL, "segment %d channel %d scale %d own input" % (seg, ch, i), own)
    _end_to_end(name, plan, got, prec, "complex", range(c["channels"]), end)
    plan.execute_resident(x, result=result)
    assert _same_bits(result.to_host(), got)
    result.free()
    plan.close()
    print("MEASURED %s-%s own %.3g %.3g %.3g end %.3g %.3g %.3g" % (name, prec, *own, *end))


MODE_RUNS = [(n, o) for n in ("F2", "F4", "F256") for o in ("amplitude", "power")]


@pytest.mark.parametrize("name, output", MODE_RUNS, ids=["%s-%s" % r for r in MODE_RUNS])
def test_full_band_amplitude_and_power(name, output):
    c = ec.CASES[name]
    plan = ec.make_plan(name, output=output)
    worst = [0.0, 0.0, 0.0]
    _end_to_end(name, plan, plan.execute(ec.recording(name)), "default", output, range(c["channels"]), worst)
    plan.close()
    print("MEASURED %s-%s end %.3g %.3g %.3g" % (name, output, *worst))


@pytest.mark.parametrize("name", list(ec.GROUP_CASES))
def test_full_band_row_groups_give_the_same_bits(name):
    """Option fullband_group only maps workgroup ids to (slot, row): 1, 8 and P1 rows per group, and 3, which divides no
    P1 and falls back to the default, against the default's 32."""
    x = ec.recording(name)
    plan = ec.make_plan(name)
    want = plan.execute(x)
    plan.close()
    assert np.abs(want).max() > 0
    for g in ec.GROUP_CASES[name]:
        other = ec.make_plan(name, fullband_group=g)
        assert _same_bits(other.execute(x), want), g
        other.close()


def test_f4_without_the_response_cache_and_in_smaller_sets():
    """F4 (sets 4 + 4 + 1): fullband_cache_mb = 0 computes every response into the scratch rows each time; a scale alone,
    in a set of two or of three (the prefetch of the next response, z_sets) is the same row as in the full plan; with
    fullband4 = 0 the two-pass kernels make the same rows from the same arithmetic."""
    name = "F4"
    x = ec.recording(name)
    plan = ec.make_plan(name)
    want = plan.execute(x)
    plan.close()
    other = ec.make_plan(name, fullband_cache_mb=0)
    assert _same_bits(other.execute(x), want)
    assert _same_bits(other.execute(x), want)                 # (and again: nothing kept from the first)
    other.close()
    for sub in ec.F4_SUBSETS:
        other = ec.make_plan(name, scales=sub)
        assert _same_bits(other.execute(x), want[:, sub]), sub
        other.close()
    for kw in (dict(), dict(fullband_cache_mb=0)):
        two = ec.make_plan(name, fullband4=0, **kw)
        got = two.execute(x)
        worst = [0.0, 0.0, 0.0]
        _end_to_end(name, two, got, "default", "complex", range(2), worst)
        print("MEASURED F4-two-pass end %.3g %.3g %.3g" % tuple(worst))
        assert _same_bits(got, want), kw
        for sub in ec.F4_SUBSETS:
            other = ec.make_plan(name, scales=sub, fullband4=0, **kw)
            assert _same_bits(other.execute(x), want[:, sub]), sub
            other.close()
        two.close()


def test_f4x_one_workgroup_makes_two_scales():
    """576 slots: launch_fullband4 splits the set of four scales over 3 workgroups, so blockIdx.y = 0 runs its loop
    twice and reuses the exchange and swap buffers; then 216 slots, split 4.  Channels 0 and 35 against the oracle;
    all 36 against the two-pass kernels (fullband4 = 0), bit for bit."""
    name = "F4x"
    x = ec.recording(name)
    plan = ec.make_plan(name, output="amplitude")
    got = plan.execute(x)
    worst = [0.0, 0.0, 0.0]
    _end_to_end(name, plan, got, "exact", "amplitude", (0, 35), worst)
    plan.close()
    print("MEASURED F4x-exact-amplitude end %.3g %.3g %.3g" % tuple(worst))
    two = ec.make_plan(name, output="amplitude", fullband4=0)
    assert _same_bits(two.execute(x), got)
    two.close()


BLOCK_RUNS = [("B1", p, "complex") for p in ec.CASES["B1"]["precisions"]] \
    + [("B1", "high", "amplitude"), ("B1", "high", "power")] + [(n, "high", "complex") for n in ("B2", "B4-1", "B4-5")]


@pytest.mark.parametrize("name, prec, output", BLOCK_RUNS, ids=["%s-%s-%s" % r for r in BLOCK_RUNS])
def test_block_convolution_end_to_end(name, prec, output):
    c = ec.CASES[name]
    x = ec.recording(name)
    plan = ec.make_plan(name, prec, output=output)
    result = plan.execute_resident(x)
    got = result.to_host()
    worst = [0.0, 0.0, 0.0]
    _end_to_end(name, plan, got, prec, output, range(c["channels"]), worst)
    plan.execute_resident(x, result=result)
    assert _same_bits(result.to_host(), got)
    result.free()
    plan.close()
    print("MEASURED %s-%s-%s end %.3g %.3g %.3g" % (name, prec, output, *worst))


def test_b1_block_requests_and_chunk_seams_give_the_same_bits():
    """execute_block at ranges that start and end one sample either side of a block edge, inside the epoch shorter than
    `back`, and on exactly one block; option bc_chunk_blocks = 2 (every pair its own launch: with b0 > 0 k_bc_scales
    finds its epoch from blk0 + lb and its spectrum from lb) and 6 -- the bits of the plan that holds every block at
    once."""
    name = "B1"
    x = ec.recording(name)
    plan = ec.make_plan(name)
    want = plan.execute(x)
    for a, ln in ec.B1_RANGES:
        assert _same_bits(plan.execute_block(x, a, ln), want[:, :, a:a + ln]), (a, ln)
    plan.close()
    for chunk in ec.CHUNKS:
        other = ec.make_plan(name, bc_chunk_blocks=chunk)
        assert _same_bits(other.execute(x), want), chunk
        for a, ln in ec.B1_RANGES:
            assert _same_bits(other.execute_block(x, a, ln), want[:, :, a:a + ln]), (chunk, a, ln)
        other.close()


DIRECT_RUNS = [(n, o) for n in ec.DIRECT_CASES for o in ec.CASES[n]["outputs"]]


@pytest.mark.parametrize("name, output", DIRECT_RUNS, ids=["%s-%s" % r for r in DIRECT_RUNS])
def test_time_domain_end_to_end(name, output):
    c = ec.CASES[name]
    x = ec.recording(name)
    plan = ec.make_plan(name, output=output)
    got = plan.execute(x)
    worst = [0.0, 0.0, 0.0]
    _end_to_end(name, plan, got, "default", output, range(c["channels"]), worst)
    assert _same_bits(plan.execute(x), got)
    plan.close()
    print("MEASURED %s-%s end %.3g %.3g %.3g" % (name, output, *worst))
