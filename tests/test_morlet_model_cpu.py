"""The float64 model of the Morlet fast path (morlet_model.cwt_decimated: the planner's own decisions, the closed-form
response of DESIGN.md "Morlet") against the literal convolution with get_wavelet(), w0 from 2 to 20, and golden G17
(the reference's kernels at w0 = 2, 4, 20).  CPU only: planning needs no device.

The model must stay within MODEL_TOL = 2.5e-6 of the truth on every row -- a quarter of the 1e-5 gate, so the device
tests of tests/test_gpu_morlet_matrix.py, which run the same layouts, leave the float32 arithmetic three quarters."""
import numpy as np
import pytest

import morlet_cases as mc
import morlet_model
from conftest import rel_err
from ghost_amd import _lib
from ghost_amd.engine import CwtPlan
from ghost_amd.wave import Morlet

G17_CASES = [(2.0, 1000.0), (4.0, 1000.0), (20.0, 1000.0)]


def _lfp(n, fs, seed):
    from ghost_amd.synthetic import lfp
    return lfp(1, n, fs, seed=seed)[0]


def _check_plan(plan, w0):
    """What the device cases rely on: below w0 = 5.6 every level's band is shifted and has no low cut; from 5.6 on no
    level is shifted; nothing is interpolated."""
    lv = mc.levels(plan)
    assert lv and plan.info["n_interp"] == 0
    if w0 < mc.TWO_SIDED_BELOW:
        assert all(l["band_shift"] > 0 and l["low_cut"] == 0 for l in lv), lv
        assert max(l["decimation"] for l in lv) <= 256               # a two-sided band stops there
    else:
        assert all(l["band_shift"] == 0 for l in lv), lv
    return lv


def _model_against_truth(name, x, fs, f, w0, rows=None, bounds=None):
    plan = CwtPlan(x.size, 1, fs, f, morlet_w0=w0, epoch_bounds=bounds, output="amplitude")
    lv = _check_plan(plan, w0)
    si = plan.scale_info()
    rows = list(range(len(f))) if rows is None else rows
    got = morlet_model.cwt_decimated(x, fs, f, w0, epoch_bounds=bounds, plan=plan, rows=rows)
    ref = mc.truth(x, fs, f, w0, rows=rows, bounds=bounds)
    err = rel_err(got, ref)
    m = si["method"][rows]
    spectral, full = m == _lib.SCALE_SPECTRAL, m == _lib.SCALE_FULLBAND
    print("%s: %d rows; worst spectral row %.2e, worst full-band row %.2e (bound %.1e); levels %s" % (
        name, len(rows), err[spectral].max() if spectral.any() else 0.0, err[full].max() if full.any() else 0.0,
        mc.MODEL_TOL, [(l["decimation"], l["halo"], l["band_shift"], l["scales"].size) for l in lv]))
    if bounds is not None:
        inside = np.zeros(x.size, bool)
        for a, b in bounds:
            inside[a:b] = True
        assert not got[:, ~inside].any()
    assert err.max() <= mc.MODEL_TOL, (name, int(np.argmax(err)), err.max())
    plan.close()
    return lv, si


@pytest.mark.parametrize("w0", mc.W0S)
def test_default_grid_70001(w0):
    fs, n = 1000.0, 70001
    f = mc.default_grid(w0, n, fs)
    lv, si = _model_against_truth("w0=%g N=70001 default grid" % w0, _lfp(n, fs, 11), fs, f, w0)
    assert (si["method"] == _lib.SCALE_SPECTRAL).sum() > f.size // 2
    if w0 == 20.0:
        assert sum(40 <= l["halo"] <= 48 for l in lv) >= 5 and all(l["halo"] <= 48 for l in lv), lv   # next to the fast kernel's limit
    if w0 <= 4.0:
        assert (si["method"] == _lib.SCALE_DIRECT).sum() >= 7


@pytest.mark.parametrize("w0, every", [(4.0, 9), (5.0, 6)])
def test_one_million_samples_wide_halo_and_full_band(w0, every):
    """N = 1e6: a shifted level with a halo beyond 48 (k_synth7's WIDE build on the device) and, below the reach of
    R = 256, full-band scales with kernels of well over 100 000 taps."""
    fs, n = 1000.0, 1000000
    f = mc.default_grid(w0, n, fs)
    rows = list(range(0, f.size, every))
    lv, si = _model_against_truth("w0=%g N=1e6 every %dth scale" % (w0, every), _lfp(n, fs, 5), fs, f, w0, rows=rows)
    assert any(l["halo"] > 48 and l["scales"].size >= 5 for l in lv), lv
    full = si["method"] == _lib.SCALE_FULLBAND
    assert full.sum() >= 15 and si["length"][full].max() > 150000
    assert {_lib.SCALE_SPECTRAL, _lib.SCALE_FULLBAND} <= set(si["method"][rows].tolist())


def test_300000_samples_every_fourth_scale():
    fs, n, w0 = 1000.0, 300000, 5.0
    f = mc.default_grid(w0, n, fs)
    lv, _ = _model_against_truth("w0=5 N=300000 every 4th scale", _lfp(n, fs, 7), fs, f, w0,
                                 rows=list(range(0, f.size, 4)))
    assert any(l["decimation"] == 256 and l["halo"] > 48 for l in lv), lv


def test_four_epochs_with_gaps():
    """Four epochs (one of 700 samples, two touching, two gaps): each with the 64-sample lead of its segment and an FFT
    length of its own; a second wide-halo level."""
    fs, w0 = 1000.0, 5.0
    lv, _ = _model_against_truth("w0=5 four epochs", _lfp(mc.FOUR_EPOCHS_N, fs, 3), fs, mc.FOUR_EPOCHS_F, w0,
                                 bounds=mc.FOUR_EPOCHS)
    assert sum(l["halo"] > 48 for l in lv) >= 1, lv


def test_shift_and_low_cut_by_w0():
    """The planner's Morlet decisions the device cases rest on, over N and w0 (host only)."""
    for w0 in mc.W0S:
        for n in (70001, 120000):
            with_plan = CwtPlan(n, 1, 1000.0, mc.default_grid(w0, n, 1000.0), morlet_w0=w0, output="power")
            lv = _check_plan(with_plan, w0)
            if w0 >= 6.0:
                assert any(l["low_cut"] > 0 for l in lv), (w0, lv)
            with_plan.close()


# ---- golden G17 --------------------------------------------------------------------------------------------------------

def test_g17_lengths_equal_the_kernels(golden):
    g = golden("G17_morlet_w0.npz")
    for w0, fs in G17_CASES:
        tag = "%g_%g" % (w0, fs)
        freqs = g["frequencies_" + tag]
        lengths = Morlet(w0=w0, fs=fs).compute_lengths(freqs / (fs / 2.0) * np.pi)
        np.testing.assert_array_equal(lengths, g["lengths_" + tag])
        np.testing.assert_array_equal(lengths, [len(g["psi_%s_%d" % (tag, k)]) for k in range(len(freqs))])
        np.testing.assert_array_equal(lengths, [morlet_model.geometry(w0, f, fs)[2] for f in freqs])
        for k in range(len(freqs)):              # this repository's class makes the reference's numbers
            np.testing.assert_allclose(Morlet(w0=w0, freq=freqs[k], fs=fs).get_wavelet(), g["psi_%s_%d" % (tag, k)],
                                       rtol=0, atol=1e-12)
        with_plan = CwtPlan(int(g["n"]), 1, fs, freqs, morlet_w0=w0)
        np.testing.assert_array_equal(with_plan.scale_info()["length"], lengths)
        with_plan.close()


def test_g17_closed_form_against_the_golden_kernels(golden):
    """Three alias terms either side, the tolerance of test_morlet_cpu.test_closed_form_against_the_golden_kernels:
    w0 = 2 (correction term 0.135 of the main one) needs no more."""
    g = golden("G17_morlet_w0.npz")
    theta = np.linspace(-np.pi, np.pi, 2001)
    for w0, fs in G17_CASES:
        tag = "%g_%g" % (w0, fs)
        worst = 0.0
        for k, f in enumerate(g["frequencies_" + tag]):
            ref = morlet_model.dtft(g["psi_%s_%d" % (tag, k)], theta)
            err = np.abs(morlet_model.response(theta, w0, f, fs) - ref).max() / np.abs(ref).max()
            worst = max(worst, err)
            assert err <= 1e-10, (w0, fs, f, err)
        print("w0=%g closed form against the DTFT of the golden kernels: worst %.2e of the peak" % (w0, worst))


def test_g17_truth_is_the_reference_convolution(golden):
    """morlet_cases.truth, what every device test compares with, is the reference's fastconv_scipy row."""
    g = golden("G17_morlet_w0.npz")
    cols = g["cols"]
    for w0, fs in G17_CASES:
        tag = "%g_%g" % (w0, fs)
        f = g["frequencies_" + tag]
        ref = mc.truth(g["x_" + tag], fs, f, w0)
        for k in range(f.size):
            peak = float(g["rowmax_%s_%d" % (tag, k)])
            assert np.abs(ref[k, cols] - g["conv_cols_%s_%d" % (tag, k)]).max() <= 1e-12 * peak
