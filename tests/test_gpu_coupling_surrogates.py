"""coupling(surrogates=...) on the MI355X (csrc/coupling_surrogates.hip, include/ghostcwt.h: gcwt_coupling_surrogates): the
kernel against the float64 model of the definition on its own input (tests/coupling_surrogates_model.py), its bits against
gcwt_coupling's and against itself, the class surface on a recording whose coupling the surrogates must find in one
channel and not in the other, and its error surface.

The bounds are derived, not measured (coupling_surrogates_model): a surrogate is made by the operations of coupling()'s
mvl (coupling_model.mvl_bound); the mean and the sd are float64 sums of the float32 surrogates, rounded once."""
import numpy as np
import pytest

import coupling_surrogates_model as sm

pytestmark = pytest.mark.gpu

FS = 1000.0
MAX_WINDOW = 2048                                           # GCWT_COUPLING_SURROGATES_MAX_WINDOW


def _resident(x, freqs, **kw):
    from ghost_amd.engine import CwtPlan
    x = np.atleast_2d(np.asarray(x, dtype=np.float32))
    plan = CwtPlan(x.shape[1], x.shape[0], FS, freqs, output="complex", **kw)
    return plan, plan.execute_resident(x)


def _run(result, phase_rows, amp_rows, window, shifts, keep=True):
    from ghost_amd import engine
    res = engine.coupling_surrogates(result, phase_rows, amp_rows, window, np.asarray(shifts, dtype=np.int64), keep=keep)
    try:
        assert (res.n_phase, res.n_amp, res.n_bins) == (phase_rows[1], amp_rows[1], -(-result.shape[2] // window))
        return res.to_host()
    finally:
        res.free()


def _mvl(result, phase_rows, amp_rows, window):
    from ghost_amd import engine
    res = engine.coupling(result, phase_rows, amp_rows, window)
    try:
        return res.to_host()["mvl"]
    finally:
        res.free()


def _shifts(window):
    return sorted(set(s for s in (0, 1, 63, 64, 65, window // 2, window - 1) if s < window))


def _compare(got, w, phase_rows, amp_rows, window, shifts, msg=""):
    """The device's four outputs against the model on the same complex64 rows ``w`` and against the float64 statistics
    of the surrogates it returned; ``shifts`` holds a 0.  Returns the worst ratios to the bounds (surrogate, mean, sd of
    the returned surrogates; mean, sd of the model)."""
    k = len(shifts)
    ref = sm.model(w, phase_rows, amp_rows, window, shifts)
    sur = got["surrogates"]
    assert sur.shape == ref["mvl"].shape and sur.dtype == np.float32, msg
    for name, dtype in (("mean", np.float32), ("sd", np.float32), ("count_ge", np.int32)):
        assert got[name].shape == ref["mean"].shape and got[name].dtype == dtype, (msg, name)
    live = np.broadcast_to(ref["s"][None, :, None] > 0, sur.shape)
    e_sur = np.abs(sur.astype(np.float64) - ref["mvl"]).max()
    assert sur.min() >= 0.0 and sur.max() <= 1.0, msg
    assert not np.any(sur[~live]), msg                     # no signal: exactly 0
    # the count, from the float32 surrogates that came back
    at0 = list(shifts).index(0)
    np.testing.assert_array_equal(got["count_ge"], (sur >= sur[at0][None]).sum(axis=0), err_msg=msg)
    assert np.all(got["count_ge"][~live[0]] == k), msg     # ... and K where there is no signal: p = 1
    # mean and sd: of the returned surrogates (rounding only), and of the model's
    s64 = sur.astype(np.float64)
    e_mean, e_sd = np.abs(got["mean"] - s64.mean(axis=0)).max(), np.abs(got["sd"] - s64.std(axis=0, ddof=1)).max()
    m_mean, m_sd = np.abs(got["mean"] - ref["mean"]).max(), np.abs(got["sd"] - ref["sd"]).max()
    b_sur = sm.surrogate_bound(window)
    ratios = (e_sur / b_sur, e_mean / sm.mean_rounding(k), e_sd / sm.sd_rounding(k), m_mean / sm.mean_bound(window, k),
              m_sd / sm.sd_bound(window, k))
    print("%s w=%d K=%d P=%s A=%s: surrogate %.3g (bound %.3g); of the returned: mean %.3g (%.3g), sd %.3g (%.3g); of the "
          "model: mean %.3g (%.3g), sd %.3g (%.3g)" % (msg, window, k, phase_rows, amp_rows, e_sur, b_sur, e_mean,
                                                       sm.mean_rounding(k), e_sd, sm.sd_rounding(k), m_mean,
                                                       sm.mean_bound(window, k), m_sd, sm.sd_bound(window, k)))
    assert max(ratios) <= 1.0, (msg, window, ratios)
    assert not np.any(got["mean"][~live[0]]) and not np.any(got["sd"][~live[0]]), msg
    return ratios


# (phase rows, amplitude rows) of a result of 14 rows; tiles are 4 phase x 8 amplitude rows
RANGES = {"disjoint": ((9, 5), (0, 9)), "overlapping": ((4, 6), (2, 7)), "identical": ((3, 4), (3, 4)),
          "one row each": ((12, 1), (1, 1)), "whole tiles": ((6, 8), (0, 8)), "everything": ((0, 14), (0, 14))}


# -- 1. the kernel against float64 NumPy on its own input -------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 3])
def test_kernel_meets_the_model_on_its_own_input(c):
    from ghost_amd.synthetic import lfp
    n = 5003                                       # a multiple of neither 32 nor any of the windows below
    x = lfp(c, n, FS, seed=11)
    kw = dict(epoch_bounds=[[0, 2000], [2700, n]]) if c == 3 else {}       # (a gap: cells without signal)
    plan, result = _resident(x, np.geomspace(200.0, 4.0, 14), **kw)
    w = result.to_host(np.complex64)
    worst = np.zeros(5)
    for window in sorted(set((2, 3, 64, 100, 256, 1000, 2048, MAX_WINDOW))):
        assert n % window and MAX_WINDOW <= n      # a short last bin everywhere: of 1 column at window 2
        shifts = _shifts(window)
        for name, (ph, am) in RANGES.items():
            got = _run(result, ph, am, window, shifts)
            worst = np.maximum(worst, _compare(got, w, ph, am, window, shifts, "C=%d %s" % (c, name)))
    print("C=%d: worst error / bound: surrogate %.3f; of the returned: mean %.3f, sd %.3f; of the model: mean %.3f, sd %.3f"
          % ((c,) + tuple(worst)))
    if c == 3:                                     # the gap's bins are there: 0 in every output, count_ge = K
        got = _run(result, (9, 5), (0, 9), 100, _shifts(100))
        for name in ("mean", "sd", "surrogates"):
            assert not np.any(got[name][..., 20:27]), name
        assert np.all(got["count_ge"][..., 20:27] == 7)
        assert np.all(got["mean"][..., :20] > 0) and np.all(got["mean"][..., 27:] > 0)
    result.free()
    plan.close()


# -- 2. bits -------------------------------------------------------------------------------------------------------------
def test_bits_of_coupling_of_a_cell_alone_of_two_runs_and_of_a_shared_shift():
    from ghost_amd.synthetic import lfp
    n, c = 20011, 3
    x = lfp(c, n, FS, seed=3)
    plan, result = _resident(x, np.geomspace(150.0, 5.0, 24))
    ph, am = (13, 10), (0, 19)                       # tiles: phase 4 + 4 + 2, amplitude 8 + 8 + 3
    names = ("mean", "sd", "count_ge", "surrogates")
    for window in (100, 1000, MAX_WINDOW):
        shifts = _shifts(window)
        a, b = _run(result, ph, am, window, shifts), _run(result, ph, am, window, shifts)
        for name in names:
            np.testing.assert_array_equal(a[name], b[name], err_msg=name)
        # L = 0 is gcwt_coupling's mvl, bit for bit (the short last bin among them)
        np.testing.assert_array_equal(a["surrogates"][shifts.index(0)], _mvl(result, ph, am, window))
        # a cell alone -- inside a tile, across tiles, in the ragged last tiles -- is the cell inside the ranges, bit for bit
        for p, q in ((0, 0), (2, 5), (3, 7), (4, 8), (5, 3), (7, 15), (8, 16), (9, 18), (1, 17), (9, 2)):
            alone = _run(result, (ph[0] + p, 1), (am[0] + q, 1), window, shifts)
            for name in names:
                np.testing.assert_array_equal(alone[name][..., 0, 0, :], a[name][..., p, q, :], err_msg=str((name, p, q)))
        # ... and inside ranges that start elsewhere, so that the cell sits in another place of another tile
        other = _run(result, (ph[0] - 3, 9), (am[0] + 5, 11), window, shifts)
        for name in names:
            np.testing.assert_array_equal(other[name][..., 3:9, 0:11, :], a[name][..., 0:6, 5:16, :], err_msg=name)
        # two lists that share shifts agree on those shifts' planes; an output left out changes nothing
        mixed = [window - 1, 5 % window, 0, 63]
        d = _run(result, ph, am, window, mixed)
        for s in (window - 1, 0, 63):
            np.testing.assert_array_equal(d["surrogates"][mixed.index(s)], a["surrogates"][shifts.index(s)], err_msg=str(s))
        e = _run(result, ph, am, window, shifts, keep=False)
        assert set(e) == {"mean", "sd", "count_ge"}
        for name in e:
            np.testing.assert_array_equal(e[name], a[name], err_msg=name)
    result.free()
    plan.close()


# -- 3. the class surface ----------------------------------------------------------------------------------------------
def test_class_surface_finds_the_coupled_channel_and_not_the_other():
    from ghost_amd.engine import surrogate_shifts
    from ghost_amd.wave import ContinuousWaveletTransform
    n, window, k = 32768, 2048, 200
    x = sm.jittered_input(n, FS)
    cwt = ContinuousWaveletTransform()
    cwt.transform(x, fs=FS, multichannel=True, output="complex", freq_limits=[4, 200], voices_per_octave=4)
    plain = cwt.coupling(phase=(4, 16), amplitude=(30, 200), window=window)
    assert all(getattr(plain, name) is None for name in ("surrogate_mean", "surrogate_sd", "z", "p", "shifts", "surrogates"))
    got = cwt.coupling(phase=(4, 16), amplitude=(30, 200), window=window, surrogates=k, seed=0, keep_surrogates=True)
    n_bins = n // window
    lead = (2, 8, 11, n_bins)
    for name, dtype in (("surrogate_mean", np.float32), ("surrogate_sd", np.float32), ("z", np.float32), ("p", np.float32),
                        ("mvl", np.float32), ("vector", np.complex64)):
        v = getattr(got, name)
        assert v.shape == lead and v.dtype == dtype, name
    assert got.surrogates.shape == (k,) + lead and got.surrogates.dtype == np.float32
    assert got.amplitude.shape == (2, 11, n_bins) and got.time.shape == (n_bins,) and got.window == window
    min_cols = int(np.ceil(FS / got.phase_frequencies.min()))                       # one period of the lowest phase row
    assert got.shifts.dtype == np.int64
    np.testing.assert_array_equal(got.shifts, surrogate_shifts(k, window, min_cols, 0))
    # vector / mvl / amplitude are the call's without surrogates, bit for bit
    for name in ("vector", "mvl", "amplitude"):
        np.testing.assert_array_equal(getattr(got, name), getattr(plain, name), err_msg=name)
    # z and p from what came back
    z, p = sm.z_and_p(got.mvl, got.surrogate_mean, got.surrogate_sd, (got.surrogates >= got.mvl[None]).sum(axis=0), k)
    np.testing.assert_array_equal(got.z, z.astype(np.float32))
    np.testing.assert_array_equal(got.p, p.astype(np.float32))
    # the cell nearest (8 Hz, 80 Hz): coupled in channel 0, not in channel 1
    p8 = int(np.argmin(np.abs(got.phase_frequencies - 8.0)))
    a80 = int(np.argmin(np.abs(got.amplitude_frequencies - 80.0)))
    z0, p0, z1, p1 = got.z[0, p8, a80], got.p[0, p8, a80], got.z[1, p8, a80], got.p[1, p8, a80]
    print("channel 0 median z %.2f, largest p %.4f; channel 1 median z %.2f, median p %.3f"
          % (np.median(z0), p0.max(), np.median(z1), np.median(p1)))
    assert np.median(z0) >= 3 and np.all(p0 <= 0.02)
    assert abs(np.median(z1)) <= 0.6 and np.median(p1) >= 0.25
    # another seed is another list; the same seed the same answer
    assert np.any(cwt.coupling(phase=(4, 16), amplitude=(30, 200), window=window, surrogates=k, seed=1).shifts != got.shifts)
    again = cwt.coupling(phase=(4, 16), amplitude=(30, 200), window=window, surrogates=k)
    assert again.surrogates is None
    for name in ("surrogate_mean", "surrogate_sd", "z", "p", "shifts"):
        np.testing.assert_array_equal(getattr(again, name), getattr(got, name), err_msg=name)


def test_composes_with_output_stride_morlet_and_the_single_channel_call():
    from ghost_amd.engine import coupling_rows, surrogate_shifts
    from ghost_amd.synthetic import lfp
    from ghost_amd.wave import ContinuousWaveletTransform, Morlet
    n = 30001
    x = lfp(4, n, FS, seed=5)
    # a strided result: min_shift counts in columns; the model on the strided coefficients
    cwt = ContinuousWaveletTransform()
    cwt.transform(x, fs=FS, freq_limits=[4, 250], multichannel=True, output="complex", output_stride=4, dtype=np.float32)
    got = cwt.coupling(phase=(4, 12), amplitude=(40, 250), window=512, surrogates=24, seed=3, keep_surrogates=True)
    cols = -(-n // 4)
    ph, am = coupling_rows((4, 12), cwt.frequencies, "phase"), coupling_rows((40, 250), cwt.frequencies, "amplitude")
    assert got.surrogates.shape == (24, 4, ph[1], am[1], -(-cols // 512))
    min_cols = int(np.ceil(FS / (4 * got.phase_frequencies.min())))
    assert 50 < min_cols < 64
    np.testing.assert_array_equal(got.shifts, surrogate_shifts(24, 512, min_cols, 3))
    w = cwt.fetch(dtype=np.float32)
    ref = sm.model(w, ph, am, 512, got.shifts)
    assert np.abs(got.surrogates - ref["mvl"]).max() <= sm.surrogate_bound(512)
    assert np.abs(got.surrogate_mean - ref["mean"]).max() <= sm.mean_bound(512, 24)
    assert np.abs(got.surrogate_sd - ref["sd"]).max() <= sm.sd_bound(512, 24)
    np.testing.assert_array_equal(np.rint(got.p.astype(np.float64) * 25 - 1), (got.surrogates >= got.mvl[None]).sum(axis=0))
    # min_shift in seconds: 0.1 s at 250 columns per second is 25 columns
    got = cwt.coupling(phase=(4, 12), amplitude=(40, 250), window=512, surrogates=24, seed=3, min_shift=0.1)
    np.testing.assert_array_equal(got.shifts, surrogate_shifts(24, 512, 25, 3))
    assert got.surrogates is None and got.z.shape == got.mvl.shape

    # a Morlet transform
    cwt = ContinuousWaveletTransform(wavelet=Morlet(w0=6))
    cwt.transform(x[:3, :20000], fs=FS, freq_limits=[5, 200], voices_per_octave=4, multichannel=True, output="complex",
                  dtype=np.float32)
    got = cwt.coupling(phase=(5, 20), amplitude=(20, 200), window=500, surrogates=16, keep_surrogates=True)
    ph, am = coupling_rows((5, 20), cwt.frequencies, "phase"), coupling_rows((20, 200), cwt.frequencies, "amplitude")
    assert got.surrogates.shape == (16, 3, ph[1], am[1], 40)
    ref = sm.model(cwt.fetch(dtype=np.float32), ph, am, 500, got.shifts)
    assert np.abs(got.surrogates - ref["mvl"]).max() <= sm.surrogate_bound(500)
    assert np.abs(got.surrogate_mean - ref["mean"]).max() <= sm.mean_bound(500, 16)
    assert np.abs(got.surrogate_sd - ref["sd"]).max() <= sm.sd_bound(500, 16)

    # the reference's single-channel call: the channel axis is dropped everywhere, axis 1 of the surrogates
    cwt = ContinuousWaveletTransform()
    cwt.transform(x[1, :20000], fs=FS, freqs=[6.0, 8.0, 10.0, 60.0, 80.0, 100.0, 120.0], output="complex", dtype=np.float32)
    got = cwt.coupling(phase=(6, 10), amplitude=(60, 120), window=1000, surrogates=10, keep_surrogates=True)
    for name in ("mvl", "surrogate_mean", "surrogate_sd", "z", "p"):
        assert getattr(got, name).shape == (3, 4, 20), name
    assert got.surrogates.shape == (10, 3, 4, 20) and got.shifts.shape == (10,)
    np.testing.assert_array_equal(got.shifts, surrogate_shifts(10, 1000, int(np.ceil(FS / 6.0)), 0))
    w = cwt.fetch(dtype=np.float32)
    assert w.shape == (7, 20000)
    ref = sm.model(w[None], (0, 3), (3, 4), 1000, got.shifts)
    assert np.abs(got.surrogates - ref["mvl"][:, 0]).max() <= sm.surrogate_bound(1000)
    assert np.abs(got.surrogate_mean - ref["mean"][0]).max() <= sm.mean_bound(1000, 10)
    z, p = sm.z_and_p(got.mvl, got.surrogate_mean, got.surrogate_sd, (got.surrogates >= got.mvl[None]).sum(axis=0), 10)
    np.testing.assert_array_equal(got.z, z.astype(np.float32))
    np.testing.assert_array_equal(got.p, p.astype(np.float32))


def test_resident_result_and_pending_fetch_are_untouched():
    from ghost_amd.synthetic import lfp
    from ghost_amd.wave import ContinuousWaveletTransform
    x = lfp(3, 9000, FS, seed=3)
    kw = dict(fs=FS, freq_limits=[5, 200], voices_per_octave=4, multichannel=True, output="complex")
    call = dict(phase=(5, 12), amplitude=(40, 200), window=1024, surrogates=12, keep_surrogates=True)
    one, twin = ContinuousWaveletTransform(), ContinuousWaveletTransform()
    one.transform(x, **kw)
    twin.transform(x, **kw)
    first = one.coupling(**call)
    np.testing.assert_array_equal(one.fetch(slice(1, 4), 100, 5000), twin.fetch(slice(1, 4), 100, 5000))
    assert one._pending is not None                  # still lazy: nothing was brought over
    np.testing.assert_array_equal(one.coefficients, twin.coefficients)
    assert one.coefficients.dtype == np.complex128
    again = one.coupling(**call)                     # ... and after the result has been brought over
    for name in ("mvl", "surrogate_mean", "surrogate_sd", "z", "p", "shifts", "surrogates"):
        np.testing.assert_array_equal(getattr(first, name), getattr(again, name), err_msg=name)
    np.testing.assert_array_equal(one.fetch(), twin.fetch())


# -- 4. the error surface on the device --------------------------------------------------------------------------------
def test_error_surface_on_the_device():
    from ghost_amd.synthetic import lfp
    from ghost_amd.wave import ContinuousWaveletTransform
    x = lfp(4, 8192, FS, seed=1)
    kw = dict(fs=FS, freq_limits=[8, 200], voices_per_octave=4)
    bands = dict(phase=(8, 16), amplitude=(40, 200))
    cwt = ContinuousWaveletTransform()
    cwt.transform(x, multichannel=True, **kw)                                     # amplitude
    with pytest.raises(ValueError, match="complex"):
        cwt.coupling(window=1024, surrogates=20, **bands)
    cwt = ContinuousWaveletTransform()
    cwt.transform(x, multichannel=True, output="complex", devices=[0, 0], **kw)   # sharded
    with pytest.raises(ValueError, match="devices"):
        cwt.coupling(window=1024, surrogates=20, **bands)
    cwt = ContinuousWaveletTransform()
    cwt.transform(x, multichannel=True, output="complex", **kw)
    with pytest.raises(ValueError, match="GCWT_COUPLING_SURROGATES_MAX_WINDOW"):
        cwt.coupling(window=MAX_WINDOW + 1, surrogates=20, **bands)
    with pytest.raises(ValueError, match=str(MAX_WINDOW)):
        cwt.coupling(window=4096, surrogates=20, **bands)
    assert cwt.coupling(window=4096, **bands).mvl.shape[-1] == 2                  # (no limit without surrogates)
    with pytest.raises(ValueError, match="window"):
        cwt.coupling(window=200, surrogates=20, **bands)                          # one period of 8.8 Hz is 114 columns
    with pytest.raises(ValueError, match="window"):
        cwt.coupling(window=1024, surrogates=20, min_shift=0.512, **bands)
    for bad in (0, -1.0, np.nan, "0.1", True):
        with pytest.raises(ValueError, match="min_shift"):
            cwt.coupling(window=1024, surrogates=20, min_shift=bad, **bands)
    for bad in (1, 4097, 20.0, True):
        with pytest.raises(ValueError, match="surrogates"):
            cwt.coupling(window=1024, surrogates=bad, **bands)
    got = cwt.coupling(window=1024, surrogates=2, **bands)
    assert got.z.shape == got.mvl.shape == (4, got.phase_frequencies.size, got.amplitude_frequencies.size, 8)
    assert got.p.min() >= 1 / 3 - 1e-6 and got.p.max() <= 1.0 and got.surrogates is None
