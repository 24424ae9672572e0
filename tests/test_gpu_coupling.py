"""coupling() on the MI355X (csrc/coupling.hip, include/ghostcwt.h: gcwt_coupling): the kernel against the float64 model
of the definition on its own input (tests/coupling_model.py), end to end against the oracle, together with
output_stride / epochs / Morlet / the single-channel call, its order and side effects, its error surface, and a shape
that exercises the tiling.

The bounds are derived, not measured (coupling_model.vector_bound / amplitude_bound / mvl_bound): the worst-case float32
rounding of the prescribed normalisation (6 roundings per term) and order -- a lane's chain of ceil(w / 64) fused
multiply-adds, a tree of 6, the divide."""
import numpy as np
import pytest

import coupling_model as pm
from oracle import ghost_oracle as orc

pytestmark = pytest.mark.gpu

FS = 1000.0


def _resident(x, freqs, **kw):
    from ghost_amd.engine import CwtPlan
    x = np.atleast_2d(np.asarray(x, dtype=np.float32))
    plan = CwtPlan(x.shape[1], x.shape[0], FS, freqs, output="complex", **kw)
    return plan, plan.execute_resident(x)


def _run(result, phase_rows, amp_rows, window):
    from ghost_amd import engine
    res = engine.coupling(result, phase_rows, amp_rows, window)
    try:
        assert (res.n_phase, res.n_amp, res.n_bins) == (phase_rows[1], amp_rows[1], -(-result.shape[2] // window))
        return res.to_host()
    finally:
        res.free()


def _compare(got, w, phase_rows, amp_rows, window, msg=""):
    """The device's three outputs against the model on the same complex64 rows ``w``; returns the worst ratios to the
    bounds (vector, mvl, amplitude)."""
    ref = pm.model(w, phase_rows, amp_rows, window)
    assert got["vector"].shape == ref["vector"].shape and got["vector"].dtype == np.complex64, msg
    assert got["mvl"].shape == ref["mvl"].shape and got["mvl"].dtype == np.float32, msg
    assert got["amplitude"].shape == ref["amplitude"].shape and got["amplitude"].dtype == np.float32, msg
    s4 = np.broadcast_to(ref["s"][:, None], ref["m"].shape)
    live, pos = s4 > 0, ref["s"] > 0
    m_dev = got["vector"].astype(np.complex128) * ref["counts"]
    e_vec = (np.abs(m_dev - ref["m"])[live] / s4[live]).max(initial=0.0)
    e_mvl = np.abs(got["mvl"].astype(np.float64) - ref["mvl"])[live].max(initial=0.0)
    e_amp = (np.abs(got["amplitude"].astype(np.float64) - ref["amplitude"])[pos] / ref["amplitude"][pos]).max(initial=0.0)
    b_vec, b_mvl, b_amp = pm.vector_bound(window), pm.mvl_bound(window), pm.amplitude_bound(window)
    print("%s w=%d P=%s A=%s: vector %.3g (bound %.3g), mvl %.3g (%.3g), amplitude %.3g (%.3g)"
          % (msg, window, phase_rows, amp_rows, e_vec, b_vec, e_mvl, b_mvl, e_amp, b_amp))
    assert e_vec <= b_vec, (msg, window, e_vec, b_vec)
    assert e_mvl <= b_mvl, (msg, window, e_mvl, b_mvl)
    assert e_amp <= b_amp, (msg, window, e_amp, b_amp)
    assert got["mvl"].min() >= 0.0 and got["mvl"].max() <= 1.0
    # cells without signal: exactly 0 in all three
    assert not np.any(got["mvl"][~live]) and not np.any(got["vector"][~live]), msg
    assert not np.any(got["amplitude"][~pos]), msg
    return e_vec / b_vec, e_mvl / b_mvl, e_amp / b_amp


def _as_dict(got):
    c = {"vector": got.vector, "mvl": got.mvl, "amplitude": got.amplitude}
    return {k: v[None] for k, v in c.items()} if got.mvl.ndim == 3 else c


# (phase rows, amplitude rows) of a result of 14 rows; tiles are 4 phase x 8 amplitude rows
RANGES = {"disjoint": ((9, 5), (0, 9)), "overlapping": ((4, 6), (2, 7)), "identical": ((3, 4), (3, 4)),
          "one row each": ((12, 1), (1, 1)), "whole tiles": ((6, 8), (0, 8)), "everything": ((0, 14), (0, 14))}


# -- 1. the kernel against float64 NumPy on its own input -------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 3, 9])
def test_kernel_meets_the_model_on_its_own_input(c):
    from ghost_amd.synthetic import lfp
    n = 5003                                       # a multiple of neither 32 nor any of the windows below
    x = lfp(c, n, FS, seed=11)
    kw = dict(epoch_bounds=[[0, 2000], [2700, n]]) if c == 3 else {}       # (a gap: cells without signal)
    plan, result = _resident(x, np.geomspace(200.0, 4.0, 14), **kw)
    assert result.pitch % 32 == 0 and result.pitch > n
    w = result.to_host(np.complex64)
    worst = np.zeros(3)
    for window in (2, 3, 64, 100, 256, 1000, n, n + 5):
        assert window == n or n % window
        for name, (ph, am) in RANGES.items():
            worst = np.maximum(worst, _compare(_run(result, ph, am, window), w, ph, am, window, "C=%d %s" % (c, name)))
    print("C=%d: worst error / bound: vector %.3f, mvl %.3f, amplitude %.3f" % ((c,) + tuple(worst)))
    if c == 3:                                     # the gap's bins are there and are exactly 0
        got = _run(result, (9, 5), (0, 9), 100)
        for name in ("vector", "mvl", "amplitude"):
            assert not np.any(got[name][..., 20:27]), name
        assert np.all(got["amplitude"][..., :20] > 0) and np.all(got["amplitude"][..., 27:] > 0)
    result.free()
    plan.close()


# -- 2. end to end against the oracle ----------------------------------------------------------------------------------
def test_class_surface_meets_the_oracle_and_the_physics():
    from ghost_amd.wave import ContinuousWaveletTransform
    n = 32768
    x = pm.coupled_input(n, FS)
    cwt = ContinuousWaveletTransform()
    cwt.transform(x, fs=FS, multichannel=True, output="complex", freq_limits=[4, 200], voices_per_octave=4)
    f = cwt.frequencies
    np.testing.assert_allclose(f, orc.frequency_grid(FS, n, freq_limits=(4, 200), voices_per_octave=4), rtol=1e-13)
    ref_w = np.stack([orc.cwt_complex(x[ch], FS, f) for ch in range(2)])
    for window in (1024, 4096):
        got = cwt.coupling(phase=(4, 16), amplitude=(30, 200), window=window)
        n_bins = -(-n // window)
        assert got.mvl.shape == (2, 8, 11, n_bins) and got.vector.shape == (2, 8, 11, n_bins) and got.amplitude.shape == (2, 11, n_bins)
        assert got.window == window and got.time.shape == (n_bins,)
        ph = (int(np.flatnonzero(f == got.phase_frequencies[0])[0]), 8)
        am = (int(np.flatnonzero(f == got.amplitude_frequencies[0])[0]), 11)
        np.testing.assert_array_equal(got.phase_frequencies, f[ph[0]:ph[0] + 8])
        np.testing.assert_array_equal(got.amplitude_frequencies, f[am[0]:am[0] + 11])
        assert got.phase_frequencies.min() >= 4 and got.phase_frequencies.max() <= 16
        assert got.amplitude_frequencies.min() >= 30 and got.amplitude_frequencies.max() <= 200
        p8 = int(np.argmin(np.abs(got.phase_frequencies - 8.0)))
        a80 = int(np.argmin(np.abs(got.amplitude_frequencies - 80.0)))
        mvl0 = float(np.median(got.mvl[0, p8, a80, 1:-1]))
        ang0 = float(np.median(np.angle(got.vector[0, p8, a80, 1:-1])))
        mvl1 = float(np.median(got.mvl[1, p8, a80, 1:-1]))
        print("window %d: channel 0 mvl %.4f angle %.4f rad, channel 1 mvl %.4f" % (window, mvl0, ang0, mvl1))
        assert mvl0 >= 0.25
        assert abs(ang0 - 1.0) <= 0.03
        assert mvl1 <= 0.05
        # every cell against the oracle, within what the transform's own gate allows
        ref = pm.model(ref_w, ph, am, window)
        gate = pm.gate_bound(ref_w, ph, am, window)
        assert gate.max() <= 2e-3, gate.max()
        ratio_dev = got.vector.astype(np.complex128) / got.amplitude.astype(np.float64)[:, None]
        err = np.abs(ratio_dev - ref["ratio"])
        bound = gate + pm.vector_bound(window)
        print("window %d: max |M/S dev - ref| %.3g, max gate bound %.3g, worst error / bound %.3f"
              % (window, err.max(), gate.max(), (err / bound).max()))
        assert np.all(err <= bound), (window, err.max(), (err / bound).max())


# -- 3. it composes with what exists -----------------------------------------------------------------------------------
def test_composes_with_output_stride_epochs_morlet_and_the_single_channel_call(golden):
    from ghost_amd.engine import coupling_rows
    from ghost_amd.synthetic import lfp
    from ghost_amd.wave import ContinuousWaveletTransform, Morlet
    n = 30001
    x = lfp(4, n, FS, seed=5)
    ts = 3.25 + np.arange(n) / FS
    # a strided result: the model on the strided coefficients; time is that of each bin's first column
    cwt = ContinuousWaveletTransform()
    cwt.transform(x, timestamps=ts, fs=FS, freq_limits=[4, 250], multichannel=True, output="complex", output_stride=4,
                  dtype=np.float32)
    got = cwt.coupling(phase=(4, 12), amplitude=(40, 250), window=64)
    cols = -(-n // 4)
    n_bins = -(-cols // 64)
    ph, am = coupling_rows((4, 12), cwt.frequencies, "phase"), coupling_rows((40, 250), cwt.frequencies, "amplitude")
    assert ph[1] > 8 and am[1] > 16
    assert got.mvl.shape == (4, ph[1], am[1], n_bins) and got.amplitude.shape == (4, am[1], n_bins) and got.window == 64
    np.testing.assert_array_equal(got.phase_frequencies, cwt.frequencies[ph[0]:ph[0] + ph[1]])
    np.testing.assert_array_equal(got.time, ts[::4][::64])
    assert got.time.shape == (n_bins,)
    w = cwt.fetch(dtype=np.float32)
    assert w.shape == (4, cwt.frequencies.size, cols) and w.dtype == np.complex64
    _compare(_as_dict(got), w, ph, am, 64, "stride 4")

    # G5's recording in two epochs (a gap in time); then with samples cut out between them: bins inside are exactly 0
    g = golden("g5_two_epochs.npz")
    xs = np.stack([g["x"], g["x"][::-1]])
    cwt = ContinuousWaveletTransform()
    cwt.transform(xs, fs=float(g["fs"]), timestamps=g["timestamps"], multichannel=True, output="complex", dtype=np.float32)
    f = cwt.frequencies
    lo, hi = (float(f.min()), float(np.sort(f)[5])), (float(np.sort(f)[-7]), float(f.max()))
    got = cwt.coupling(phase=lo, amplitude=hi, window=100)
    ph, am = coupling_rows(lo, f, "phase"), coupling_rows(hi, f, "amplitude")
    assert (ph[1], am[1]) == (6, 7)
    np.testing.assert_array_equal(got.time, np.asarray(g["timestamps"])[::100])
    _compare(_as_dict(got), cwt.fetch(dtype=np.float32), ph, am, 100, "G5")
    plan, result = _resident(xs, g["frequencies"][:30], epoch_bounds=[[0, 5900], [6100, 10000]])
    out = _run(result, (20, 10), (0, 12), 64)
    inside = [m for m in range(out["amplitude"].shape[-1]) if 64 * m >= 5900 and 64 * (m + 1) <= 6100]
    assert inside == [93, 94]
    for name in ("vector", "mvl", "amplitude"):
        assert not np.any(out[name][..., inside]), name
        assert np.all(out[name][..., [91, 96]] != 0), name
    _compare(out, result.to_host(np.complex64), (20, 10), (0, 12), 64, "G5 with a gap")
    result.free()
    plan.close()

    # a Morlet transform
    cwt = ContinuousWaveletTransform(wavelet=Morlet(w0=6))
    cwt.transform(x[:3, :20000], fs=FS, freq_limits=[5, 200], voices_per_octave=4, multichannel=True, output="complex",
                  dtype=np.float32)
    got = cwt.coupling(phase=(5, 20), amplitude=(20, 200), window=500)
    ph, am = coupling_rows((5, 20), cwt.frequencies, "phase"), coupling_rows((20, 200), cwt.frequencies, "amplitude")
    assert got.mvl.shape == (3, ph[1], am[1], 40)
    _compare(_as_dict(got), cwt.fetch(dtype=np.float32), ph, am, 500, "Morlet")

    # the reference's single-channel call: the channel axis is dropped; ascending freqs=
    cwt = ContinuousWaveletTransform()
    cwt.transform(x[1, :20000], fs=FS, freqs=[6.0, 8.0, 10.0, 60.0, 80.0, 100.0, 120.0], output="complex", dtype=np.float32)
    np.testing.assert_array_equal(cwt.frequencies, [6.0, 8.0, 10.0, 60.0, 80.0, 100.0, 120.0])
    got = cwt.coupling(phase=(6, 10), amplitude=(60, 120), window=1000)
    assert got.mvl.shape == (3, 4, 20) and got.vector.shape == (3, 4, 20) and got.amplitude.shape == (4, 20)
    assert got.mvl.dtype == np.float32 and got.vector.dtype == np.complex64
    np.testing.assert_array_equal(got.phase_frequencies, [6.0, 8.0, 10.0])
    np.testing.assert_array_equal(got.amplitude_frequencies, [60.0, 80.0, 100.0, 120.0])
    w = cwt.fetch(dtype=np.float32)
    assert w.shape == (7, 20000)
    _compare(_as_dict(got), w[None], (0, 3), (3, 4), 1000, "single channel")


# -- 4. order, determinism and side effects ----------------------------------------------------------------------------
def test_order_determinism_and_side_effects():
    from ghost_amd.synthetic import lfp
    from ghost_amd.wave import ContinuousWaveletTransform
    n, c = 20011, 3
    x = lfp(c, n, FS, seed=3)
    plan, result = _resident(x, np.geomspace(150.0, 5.0, 24))
    ph, am = (13, 10), (0, 19)                       # tiles: phase 4 + 4 + 2, amplitude 8 + 8 + 3
    for window in (100, 1000):
        a, b = _run(result, ph, am, window), _run(result, ph, am, window)
        for name in ("vector", "mvl", "amplitude"):
            np.testing.assert_array_equal(a[name], b[name], err_msg=name)
        # a cell alone -- inside a tile, across tiles, in the ragged last tiles -- is the cell inside the ranges, bit for bit
        for p, q in ((0, 0), (2, 5), (3, 7), (4, 8), (5, 3), (7, 15), (8, 16), (9, 18), (1, 17), (9, 2)):
            alone = _run(result, (ph[0] + p, 1), (am[0] + q, 1), window)
            np.testing.assert_array_equal(alone["vector"][:, 0, 0], a["vector"][:, p, q], err_msg=str((p, q)))
            np.testing.assert_array_equal(alone["mvl"][:, 0, 0], a["mvl"][:, p, q], err_msg=str((p, q)))
            np.testing.assert_array_equal(alone["amplitude"][:, 0], a["amplitude"][:, q], err_msg=str((p, q)))
        # ... and inside ranges that start elsewhere, so that the cell sits in another place of another tile
        other = _run(result, (ph[0] - 3, 9), (am[0] + 5, 11), window)
        np.testing.assert_array_equal(other["vector"][:, 3:9, 0:11], a["vector"][:, 0:6, 5:16])
        np.testing.assert_array_equal(other["mvl"][:, 3:9, 0:11], a["mvl"][:, 0:6, 5:16])
        np.testing.assert_array_equal(other["amplitude"], a["amplitude"][:, 5:16])
    result.free()
    plan.close()

    # the resident result and the pending lazy fetch are as they were
    kw = dict(fs=FS, freq_limits=[5, 200], voices_per_octave=4, multichannel=True, output="complex")
    one, twin = ContinuousWaveletTransform(), ContinuousWaveletTransform()
    one.transform(x[:3, :9000], **kw)
    twin.transform(x[:3, :9000], **kw)
    first = one.coupling(phase=(5, 12), amplitude=(40, 200), window=128)
    np.testing.assert_array_equal(one.fetch(slice(1, 4), 100, 5000), twin.fetch(slice(1, 4), 100, 5000))
    assert one._pending is not None                  # still lazy: nothing was brought over
    np.testing.assert_array_equal(one.coefficients, twin.coefficients)
    assert one.coefficients.dtype == np.complex128
    again = one.coupling(phase=(5, 12), amplitude=(40, 200), window=128)    # ... and after the result has been brought over
    np.testing.assert_array_equal(first.vector, again.vector)
    np.testing.assert_array_equal(first.mvl, again.mvl)
    np.testing.assert_array_equal(one.fetch(), twin.fetch())


# -- 5. the error surface on the device --------------------------------------------------------------------------------
def test_error_surface_on_the_device():
    from ghost_amd.synthetic import lfp
    from ghost_amd.wave import ContinuousWaveletTransform
    x = lfp(4, 8192, FS, seed=1)
    kw = dict(fs=FS, freq_limits=[8, 200], voices_per_octave=4)
    bands = dict(phase=(8, 16), amplitude=(40, 200))
    cwt = ContinuousWaveletTransform()
    cwt.transform(x, multichannel=True, **kw)                                     # amplitude
    with pytest.raises(ValueError, match="complex"):
        cwt.coupling(window=64, **bands)
    cwt = ContinuousWaveletTransform()
    cwt.transform(x, multichannel=True, output="complex", devices=[0, 0], **kw)   # sharded
    with pytest.raises(ValueError, match="devices"):
        cwt.coupling(window=64, **bands)
    cwt = ContinuousWaveletTransform()
    cwt.transform(x, multichannel=True, output="complex", **kw)
    with pytest.raises(ValueError, match="window"):
        cwt.coupling(window=1, **bands)
    with pytest.raises(ValueError, match="phase"):
        cwt.coupling(phase=(1, 4), amplitude=(40, 200), window=64)                # a band with no rows
    with pytest.raises(ValueError, match="amplitude"):
        cwt.coupling(phase=(8, 16), amplitude=(300, 400), window=64)
    with pytest.raises(ValueError, match="amplitude"):
        cwt.coupling(phase=(8, 16), amplitude=(200, 40), window=64)
    with pytest.raises(TypeError):
        cwt.coupling(phase=(8, 16), window=64)
    with pytest.raises(TypeError):
        cwt.coupling(amplitude=(40, 200), window=64)
    with pytest.raises(TypeError):
        cwt.coupling(**bands)
    with pytest.raises(TypeError):
        cwt.coupling((8, 16), (40, 200), 64)
    got = cwt.coupling(window=64, **bands)
    assert got.mvl.shape == (4, got.phase_frequencies.size, got.amplitude_frequencies.size, 128)


# -- 6. a shape that exercises the tiles -------------------------------------------------------------------------------
def test_sixteen_channels_twelve_by_twenty_rows():
    from ghost_amd.synthetic import lfp
    c, n, window = 16, 1 << 18, 1000
    x = lfp(c, n, FS, seed=21)
    plan, result = _resident(x, np.geomspace(200.0, 2.0, 40))
    ph, am = (26, 12), (2, 20)
    got = _run(result, ph, am, window)
    n_bins = -(-n // window)
    assert got["mvl"].shape == (16, 12, 20, n_bins) and got["vector"].shape == (16, 12, 20, n_bins)
    assert got["amplitude"].shape == (16, 20, n_bins)
    assert got["mvl"].min() >= 0.0 and got["mvl"].max() <= 1.0
    rng = np.random.default_rng(6)
    cells = [(int(rng.integers(16)), int(rng.integers(12)), int(rng.integers(20)), int(rng.integers(n_bins))) for _ in range(200)]
    cells += [(0, 0, 0, n_bins - 1), (15, 11, 19, n_bins - 1)]                    # the short last bin
    worst = np.zeros(3)
    for ch, p, q, m in cells:
        rows = [result.to_host(np.complex64, scales=r, start=m * window, stop=(m + 1) * window)[ch, 0]
                for r in (ph[0] + p, am[0] + q)]
        ref = pm.model(np.stack(rows)[None], (0, 1), (1, 1), window)
        cnt = min(window, n - m * window)
        assert ref["counts"].tolist() == [cnt]
        s = ref["s"][0, 0, 0]
        errs = (abs(complex(got["vector"][ch, p, q, m]) * cnt - ref["m"][0, 0, 0, 0]) / s / pm.vector_bound(window),
                abs(float(got["mvl"][ch, p, q, m]) - ref["mvl"][0, 0, 0, 0]) / pm.mvl_bound(window),
                abs(float(got["amplitude"][ch, q, m]) - ref["amplitude"][0, 0, 0]) / ref["amplitude"][0, 0, 0]
                / pm.amplitude_bound(window))
        worst = np.maximum(worst, errs)
        assert max(errs) <= 1.0, (ch, p, q, m, errs)
    print("16 channels, 12 x 20 rows: worst error / bound: vector %.3f, mvl %.3f, amplitude %.3f" % tuple(worst))
    result.free()
    plan.close()
