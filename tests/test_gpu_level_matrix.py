"""The front end stage by stage, every case of tests/level_cases.py on the device (GPU): the stored spectrum, x_R of
every level and the block spectra of every segment and channel against float64 models of the same operation, each stage
on its own input -- x_R from the spectrum fetched from the device, the block spectra from the x_R fetched from the
device -- so that a failure names the pass that is wrong; x_R also end to end, and a few final rows against
decimated_model.cwt_decimated, which ties the stages to the result.

Gates: the project's own (tests/test_gpu_stages.py) on max|err| / max|ref| -- 2e-6 on the spectrum, 3e-6 on x_R and the
block spectra, 1e-5 on final rows -- and on rms(err) / rms(ref) four times what scipy.fft makes of the same transform in
single precision (level_cases.RMS_FACTOR), computed here on the same data.  profiles/level_matrix.md has what was
measured."""
import numpy as np
import pytest

import level_cases as lc
from conftest import rel_err
from decimated_model import cwt_decimated

pytestmark = pytest.mark.gpu


class _Options:
    """Library switches for the plans made inside the ``with`` (they are read when a plan is created)."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        from ghost_amd.engine import set_option
        for k, v in self.kw.items():
            set_option(k, v)

    def __exit__(self, *exc):
        from ghost_amd.engine import set_option
        for k in self.kw:
            set_option(k, None)


def _fetch_spectrum(plan, ch, seg, p1, ncol):
    return plan.debug_fetch(0, channel=ch, epoch=seg).reshape(p1, lc.ROW)[:, :ncol].astype(np.complex128)


def _worse(worst, key, mx, rms, rms_ref):
    w = worst.setdefault(key, [0.0, 0.0, 0.0])
    w[0], w[1], w[2] = max(w[0], mx), max(w[1], rms), max(w[2], rms / rms_ref if rms_ref > 0 else 0.0)


def _gate(got, ref, single, hard, what):
    """Both gates of one comparison; returns (max, rms, rms of the single-precision reference)."""
    mx, rms = lc.compare(got, ref)
    rms_ref = lc.compare(single, ref)[1]
    print("    %s: max %.3g rms %.3g (single precision %.3g: %.2f x)" % (what, mx, rms, rms_ref, rms / rms_ref))
    assert mx < hard, (what, mx)
    assert rms <= lc.RMS_FACTOR * rms_ref, (what, rms, rms_ref)
    return mx, rms, rms_ref


def _row_choice(plan, n):
    """The scales whose final rows are compared: one per decimated level with a kernel below 2^20 taps (the model's
    gain is a NumPy sum over the kernel's kept bins), three levels of them -- first, middle, last -- above 300 000
    samples, where a row of the model costs a second."""
    from decimated_model import level_of_scale
    si, lof = plan.scale_info(), level_of_scale(plan)
    rows = []
    for l in sorted(set(lof[lof >= 0].tolist())):
        cand = [i for i in np.flatnonzero(lof == l) if si["length"][i] < (1 << 20)]
        if cand:
            rows.append(int(cand[len(cand) // 2]))
    if n > 300000 and len(rows) > 3:
        rows = [rows[0], rows[len(rows) // 2], rows[-1]]
    return rows


def _check_stages(name, prec, tag, spectrum_too, rows_too=True):
    c = lc.CASES[name]
    x = lc.recording(name)
    plan = lc.make_plan(name, prec)
    result = plan.execute_resident(x)
    p, p_store, p1, a, ncol = lc.geometry(plan)
    segs = plan.segments()
    worst = {}
    last_xr = {}
    for seg, (start, stop, _) in enumerate(segs):
        levels = plan.debug_levels(epoch=seg)
        for ch in range(c["channels"]):
            s_in = lc.segment_input(x[ch], start, stop)
            X, X32 = lc.spectrum(s_in, p), lc.spectrum(s_in, p, single=True)
            got_s = _fetch_spectrum(plan, ch, seg, p1, ncol)
            print("  %s segment %d channel %d" % (tag, seg, ch))
            if spectrum_too:                                                                      # (a)
                _worse(worst, "spectrum", *_gate(got_s, lc.stored(X, p1, ncol), lc.stored(X32, p1, ncol),
                                                 lc.GATE_SPECTRUM, "spectrum"))
            xlo_dev, xlo, xlo32 = lc.natural(got_s), X[:p1 * ncol], X32[:p1 * ncol]
            for l, lv in enumerate(levels):
                xr = plan.debug_fetch(1, channel=ch, epoch=seg, level=l)
                if ch == c["channels"] - 1:
                    last_xr[(seg, l)] = xr
                what = "x_R level %d R %d" % (l, lv["decimation"])
                sl = lc.level_slice(xlo_dev, p, lv)                                               # (b) on its own input
                _worse(worst, (l, lv["decimation"], "own"),
                       *_gate(xr, lc.xr_of_slice(sl), lc.xr_of_slice(sl, single=True), lc.GATE_XR, what + " own input"))
                ref = lc.xr_model(xlo, p, lv)                                                     # (b) end to end
                single = lc.xr_of_slice(lc.level_slice(xlo32, p, lv), single=True)
                _worse(worst, (l, lv["decimation"], "end"), *_gate(xr, ref, single, lc.GATE_XR, what + " end to end"))
    # (d) a second execute gives the same bits
    plan.execute_resident(x, result=result)
    for (seg, l), xr in last_xr.items():
        again = plan.debug_fetch(1, channel=c["channels"] - 1, epoch=seg, level=l)
        assert np.array_equal(again.view(np.uint32), xr.view(np.uint32)), (seg, l)
    # (e) final rows of one channel against the float64 model of the whole path
    if rows_too:
        ch = c["channels"] - 1
        rows = _row_choice(plan, c["n"])
        assert rows
        model_plan = lc.make_plan(name, prec, n_channels=1)
        ref = cwt_decimated(x[ch], c["fs"], c["f"], lc.epochs_of(name), c["gamma"], c["beta"], plan=model_plan, rows=rows)
        for i in rows:
            got = result.to_host(scales=i)[ch, 0]
            err = float(rel_err(got, ref[i]))
            print("  %s row %d: %.3g" % (tag, i, err))
            worst["rows"] = [max(worst.get("rows", [0.0])[0], err)]
            assert err < lc.GATE_ROWS, (i, err)
    result.free()
    for key, w in worst.items():
        print("MEASURED %s %s %s" % (tag, key, " ".join("%.3g" % v for v in w)))
    plan.close()


@pytest.mark.parametrize("name, prec", lc.RUNS, ids=["%s-%s" % r for r in lc.RUNS])
def test_front_end_stages(name, prec):
    """(a) the stored spectrum -- in float32 (precision = 'fast') on every case that runs so, in float64 where
    test_channel_means_taken_inside_the_forward_passes does not reach: a full-band plan, launch batches with and without
    leads, long mode -- mirrored rows included; (b) x_R of every level from the device's own spectrum and end to end;
    (d) the bits of a second execute; (e) final rows."""
    _check_stages(name, prec, "%s-%s" % (name, prec), prec == "fast" or name in lc.DEFAULT_SPECTRUM_CASES)


@pytest.mark.parametrize("name, prec", [(n, pr) for n in lc.SLOW_FFT_CASES for pr in ("default", "fast")],
                         ids=["%s-%s" % (n, pr) for n in lc.SLOW_FFT_CASES for pr in ("default", "fast")])
def test_front_end_stages_with_the_generic_kernels(name, prec):
    """Option slow_fft = 1: the generic radix-2 row and column kernels at every size meet the same gates.  The forward
    transform is then float32 under either precision (the float64 one has no generic form); the default keeps its low
    cut."""
    with _Options(slow_fft=1):
        _check_stages(name, prec, "%s-%s-slow" % (name, prec), True, rows_too=prec == "default")


@pytest.mark.parametrize("name", lc.BLOCK_CASES)
def test_block_spectra(name):
    """(c) every block spectrum of every level, segment and channel, from the x_R the device holds (option fuse_blocks = 0:
    the separate block pass, so that the array exists)."""
    c = lc.CASES[name]
    x = lc.recording(name)
    with _Options(fuse_blocks=0):
        plan = lc.make_plan(name)
    plan.execute(x)
    p = lc.geometry(plan)[0]
    worst = {}
    for seg in range(len(plan.segments())):
        for l, lv in enumerate(plan.debug_levels(epoch=seg)):
            for ch in range(c["channels"]):
                xr = plan.debug_fetch(1, channel=ch, epoch=seg, level=l).astype(np.complex128)
                xb = plan.debug_fetch(2, channel=ch, epoch=seg, level=l).reshape(lv["nblk"], lc.BLOCK)
                _worse(worst, (l, lv["decimation"], lv["nblk"]),
                       *_gate(xb, lc.blocks_model(xr, p, lv), lc.blocks_model(xr, p, lv, single=True), lc.GATE_BLOCKS,
                              "blocks segment %d level %d R %d channel %d" % (seg, l, lv["decimation"], ch)))
    for key, w in worst.items():
        print("MEASURED %s-blocks %s %s" % (name, key, " ".join("%.3g" % v for v in w)))
    plan.close()


@pytest.mark.parametrize("name", lc.STREAM_CASES)
def test_levels_on_one_stream_give_the_bits_of_three(name):
    """(d) level_streams = 0 runs every level pass on the plan's own stream; the default shares them among three, and
    shifted levels on one stream share that stream's slice buffer (case 8).  The same x_R, bit for bit."""
    c = lc.CASES[name]
    x = lc.recording(name)
    plan = lc.make_plan(name)
    with _Options(level_streams=0):
        serial = lc.make_plan(name)
    assert len(plan.debug_levels()) > 2                       # (api.cpp: side streams from three levels on)
    plan.execute_resident(x).free()
    serial.execute_resident(x).free()
    for l in range(len(plan.debug_levels())):
        for ch in range(c["channels"]):
            a = plan.debug_fetch(1, channel=ch, level=l)
            b = serial.debug_fetch(1, channel=ch, level=l)
            assert np.abs(a).max() > 0
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (l, ch)
    plan.close()
    serial.close()
