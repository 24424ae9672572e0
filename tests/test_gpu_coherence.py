"""coherence() on the MI355X (csrc/coherence.hip, include/ghostcwt.h: gcwt_coherence): the kernel against the float64
model of the definition on its own input (tests/coherence_model.py), end to end against the oracle, together with
output_stride / epochs / Morlet, its order and side effects, its error surface, and a shape that exercises the tiling.

The bounds are derived, not measured (coherence_model.gamma_bound / power_bound): the worst-case float32 rounding of the
prescribed order -- a lane's chain of 2 ceil(w / 64) fused multiply-adds, a tree of 6, the divide and the root."""
import numpy as np
import pytest

import coherence_model as cm
from oracle import ghost_oracle as orc

pytestmark = pytest.mark.gpu

FS = 1000.0


def _resident(x, freqs, **kw):
    from ghost_amd.engine import CwtPlan
    x = np.atleast_2d(np.asarray(x, dtype=np.float32))
    plan = CwtPlan(x.shape[1], x.shape[0], FS, freqs, output="complex", **kw)
    return plan, plan.execute_resident(x)


def _run(result, pairs, window):
    from ghost_amd import engine
    res = engine.coherence(result, pairs, window)
    try:
        assert (res.n_pairs, res.n_bins) == (len(pairs), -(-result.shape[2] // window))
        return res.to_host()
    finally:
        res.free()


def _compare(got, w, pairs, window, msg=""):
    """The device's three outputs against the model on the same complex64 rows ``w``; returns the worst ratios to the
    bounds (gamma, coherence, power)."""
    ref = cm.model(w, pairs, window)
    pairs = np.asarray(pairs).reshape(-1, 2)
    assert got["cross"].shape == ref["cross"].shape and got["cross"].dtype == np.complex64, msg
    assert got["coherence"].shape == ref["coherence"].shape and got["coherence"].dtype == np.float32, msg
    assert got["power"].shape == ref["power"].shape and got["power"].dtype == np.float32, msg
    live = ref["sxx"][pairs[:, 0]] * ref["sxx"][pairs[:, 1]] > 0
    g_dev = cm.gamma_of(got["cross"], got["power"], pairs)
    bound = cm.gamma_bound(window)
    e_gamma = np.abs(g_dev - ref["gamma"])[live].max(initial=0.0)
    e_coh = np.abs(got["coherence"].astype(np.float64) - ref["coherence"])[live].max(initial=0.0)
    pos = ref["power"] > 0
    e_pow = (np.abs(got["power"].astype(np.float64) - ref["power"])[pos] / ref["power"][pos]).max(initial=0.0)
    print("%s w=%d P=%d: gamma %.3g (bound %.3g), coherence %.3g (%.3g), power %.3g (%.3g)"
          % (msg, window, len(pairs), e_gamma, bound, e_coh, 2 * bound, e_pow, cm.power_bound(window)))
    assert e_gamma <= bound, (msg, window, e_gamma, bound)
    assert e_coh <= 2 * bound, (msg, window, e_coh, 2 * bound)
    assert e_pow <= cm.power_bound(window), (msg, window, e_pow)
    assert got["coherence"].min() >= 0.0 and got["coherence"].max() <= 1.0
    # cells without signal: exactly 0 in all three
    assert not np.any(got["coherence"][~live]) and not np.any(got["cross"][~live]), msg
    assert not np.any(got["power"][~pos]), msg
    return e_gamma / bound, e_coh / (2 * bound), e_pow / cm.power_bound(window)


def _mixed_list(c, rng):
    """An explicit list: repeats, both orders of a pair, pairs across and inside tiles."""
    base = [(0, c - 1), (c - 1, 0), (0, c - 1), (1, 0), (0, 1)]
    for _ in range(5):
        a, b = rng.choice(c, 2, replace=False) if c > 2 else (1, 0)
        base.append((int(a), int(b)))
    return np.array(base, dtype=np.int64)


# -- 1. the kernel against float64 NumPy on its own input -------------------------------------------------------------
@pytest.mark.parametrize("c", [2, 3, 9, 17])
def test_kernel_meets_the_model_on_its_own_input(c):
    from ghost_amd.synthetic import lfp
    n = 5003                                       # a multiple of neither 32 nor any of the windows below
    x = lfp(c, n, FS, seed=11)
    kw = dict(epoch_bounds=[[0, 2000], [2700, n]]) if c == 3 else {}       # (a gap: cells without signal)
    plan, result = _resident(x, np.geomspace(200.0, 4.0, 6), **kw)
    assert result.pitch % 32 == 0 and result.pitch > n
    w = result.to_host(np.complex64)
    rng = np.random.default_rng(c)
    modes = {"all": cm.all_pairs(c), "seed": cm.seed_pairs(c // 2, c), "list": _mixed_list(c, rng)}
    for window in (2, 3, 64, 100, 256, 1000, n, n + 5):
        assert window == n or n % window
        for name, pairs in modes.items():
            _compare(_run(result, pairs, window), w, pairs, window, "C=%d %s" % (c, name))
    if c == 3:                                     # the gap's bins are there and are exactly 0
        got = _run(result, modes["all"], 100)
        assert not np.any(got["power"][:, :, 20:27]) and not np.any(got["coherence"][:, :, 20:27])
        assert np.all(got["power"][:, :, :20] > 0) and np.all(got["power"][:, :, 27:] > 0)
    result.free()
    plan.close()


# -- 2. end to end against the oracle ----------------------------------------------------------------------------------
def test_class_surface_meets_the_oracle_and_the_physics():
    from ghost_amd.wave import ContinuousWaveletTransform
    n = 32768
    x = cm.three_channel_input(n, FS)
    cwt = ContinuousWaveletTransform()
    cwt.transform(x, fs=FS, multichannel=True, output="complex", freq_limits=[2, 300], voices_per_octave=4)
    f = cwt.frequencies
    np.testing.assert_allclose(f, orc.frequency_grid(FS, n, freq_limits=(2, 300), voices_per_octave=4), rtol=1e-13)
    ref_w = np.stack([orc.cwt_complex(x[ch], FS, f) for ch in range(3)])
    peak = np.abs(ref_w).max(axis=-1, keepdims=True)
    r8, r100 = int(np.argmin(np.abs(f - 8.0))), int(np.argmin(np.abs(f - 100.0)))
    for window in (256, 1024):
        got = cwt.coherence(window=window)
        assert got.pairs.tolist() == [[0, 1], [0, 2], [1, 2]]
        ref = cm.model(ref_w, got.pairs, window)
        strong = np.sqrt(ref["power"]) >= 1e-2 * peak                      # both channels' bin RMS against the row's peak
        cells = strong[got.pairs[:, 0]] & strong[got.pairs[:, 1]]
        left_out = 1.0 - cells.mean()
        err = np.abs(cm.gamma_of(got.cross, got.power, got.pairs) - ref["gamma"])[cells].max()
        print("window %d: max |gamma_dev - gamma_ref| %.3g over %.2f %% of the cells" % (window, err, 100 * cells.mean()))
        assert left_out <= 0.01, left_out
        assert err <= 4e-3, (window, err)
        if window == 256:
            coh01 = float(np.median(got.coherence[0, r8]))
            lag01 = float(np.median(np.angle(got.cross[0, r8])))
            coh02 = float(np.median(got.coherence[1, r100]))
            print("coherence (0,1) at 8 Hz %.4f, angle %.4f rad, coherence (0,2) at 100 Hz %.4f" % (coh01, lag01, coh02))
            assert coh01 >= 0.99
            assert abs(lag01 - 0.7) <= 0.02
            assert coh02 <= 0.2


# -- 3. it composes with what exists -----------------------------------------------------------------------------------
def test_composes_with_output_stride_epochs_and_morlet(golden):
    from ghost_amd.synthetic import lfp
    from ghost_amd.wave import ContinuousWaveletTransform, Morlet
    n = 30001
    x = lfp(4, n, FS, seed=5)
    ts = 3.25 + np.arange(n) / FS
    # a strided result: the model on the strided coefficients; time is that of each bin's first column
    cwt = ContinuousWaveletTransform()
    cwt.transform(x, timestamps=ts, fs=FS, freq_limits=[4, 250], multichannel=True, output="complex", output_stride=4,
                  dtype=np.float32)
    got = cwt.coherence(window=64)
    cols = -(-n // 4)
    n_bins = -(-cols // 64)
    s = cwt.frequencies.size
    assert got.coherence.shape == (6, s, n_bins) and got.cross.shape == (6, s, n_bins) and got.power.shape == (4, s, n_bins)
    assert got.pairs.shape == (6, 2) and got.window == 64
    np.testing.assert_array_equal(got.frequencies, cwt.frequencies)
    np.testing.assert_array_equal(got.time, ts[::4][::64])
    assert got.time.shape == (n_bins,)
    w = cwt.fetch(dtype=np.float32)
    assert w.shape == (4, s, cols) and w.dtype == np.complex64
    _compare({"coherence": got.coherence, "cross": got.cross, "power": got.power}, w, got.pairs, 64, "stride 4")

    # G5's recording in two epochs (a gap in time); then with samples cut out between them: bins inside are exactly 0
    g = golden("g5_two_epochs.npz")
    xs = np.stack([g["x"], g["x"][::-1]])
    cwt = ContinuousWaveletTransform()
    cwt.transform(xs, fs=float(g["fs"]), timestamps=g["timestamps"], multichannel=True, output="complex", dtype=np.float32)
    got = cwt.coherence(seed=1, window=100)
    assert got.pairs.tolist() == [[1, 0]]
    np.testing.assert_array_equal(got.time, np.asarray(g["timestamps"])[::100])
    _compare({"coherence": got.coherence, "cross": got.cross, "power": got.power}, cwt.fetch(dtype=np.float32), got.pairs,
             100, "G5")
    plan, result = _resident(xs, g["frequencies"][:30], epoch_bounds=[[0, 5900], [6100, 10000]])
    out = _run(result, cm.all_pairs(2), 64)
    inside = [m for m in range(out["power"].shape[-1]) if 64 * m >= 5900 and 64 * (m + 1) <= 6100]
    assert inside == [93, 94]
    for name in ("coherence", "cross", "power"):
        assert not np.any(out[name][..., inside]), name
        assert np.all(out[name][..., [91, 96]] != 0), name
    _compare(out, result.to_host(np.complex64), cm.all_pairs(2), 64, "G5 with a gap")
    result.free()
    plan.close()

    # a Morlet transform
    cwt = ContinuousWaveletTransform(wavelet=Morlet(w0=6))
    cwt.transform(x[:3, :20000], fs=FS, freq_limits=[5, 200], voices_per_octave=4, multichannel=True, output="complex",
                  dtype=np.float32)
    got = cwt.coherence([[2, 0], [0, 1]], window=500)
    assert got.coherence.shape == (2, cwt.frequencies.size, 40)
    _compare({"coherence": got.coherence, "cross": got.cross, "power": got.power}, cwt.fetch(dtype=np.float32), got.pairs,
             500, "Morlet")


# -- 4. order, determinism and side effects ----------------------------------------------------------------------------
def test_order_determinism_and_side_effects():
    from ghost_amd.synthetic import lfp
    from ghost_amd.wave import ContinuousWaveletTransform
    n, c = 20011, 17
    x = lfp(c, n, FS, seed=3)
    plan, result = _resident(x, np.geomspace(150.0, 5.0, 5))
    everything = cm.all_pairs(c)
    for window in (100, 1000):
        a, b = _run(result, everything, window), _run(result, everything, window)
        for name in ("coherence", "cross", "power"):
            np.testing.assert_array_equal(a[name], b[name], err_msg=name)
        # a pair alone -- inside a tile, across tiles, with the ragged last tile -- is the pair among all, bit for bit
        for pair in ((0, 1), (2, 7), (3, 12), (7, 8), (5, 16), (15, 16), (8, 15)):
            row = int(np.flatnonzero((everything == pair).all(axis=1))[0])
            alone = _run(result, [pair], window)
            np.testing.assert_array_equal(alone["cross"][0], a["cross"][row], err_msg=str(pair))
            np.testing.assert_array_equal(alone["coherence"][0], a["coherence"][row], err_msg=str(pair))
            np.testing.assert_array_equal(alone["power"], a["power"], err_msg=str(pair))
            # the other order: the conjugate cross, the same coherence
            back = _run(result, [pair[::-1]], window)
            bound = cm.gamma_bound(window)
            norm = np.sqrt(a["power"][pair[0]].astype(np.float64) * a["power"][pair[1]])
            assert (np.abs(back["cross"][0] - np.conj(alone["cross"][0])) <= bound * norm).all()
            assert np.abs(back["coherence"][0].astype(np.float64) - alone["coherence"][0]).max() <= 2 * bound
        seed = _run(result, cm.seed_pairs(9, c), window)
        for k, (s_, o) in enumerate(cm.seed_pairs(9, c)):
            if o > 9:
                row = int(np.flatnonzero((everything == (9, o)).all(axis=1))[0])
                np.testing.assert_array_equal(seed["cross"][k], a["cross"][row])
    result.free()
    plan.close()

    # the resident result and the pending lazy fetch are as they were
    kw = dict(fs=FS, freq_limits=[5, 200], voices_per_octave=4, multichannel=True, output="complex")
    one, twin = ContinuousWaveletTransform(), ContinuousWaveletTransform()
    one.transform(x[:3, :9000], **kw)
    twin.transform(x[:3, :9000], **kw)
    first = one.coherence(window=128)
    np.testing.assert_array_equal(one.fetch(slice(1, 4), 100, 5000), twin.fetch(slice(1, 4), 100, 5000))
    assert one._pending is not None                  # still lazy: nothing was brought over
    np.testing.assert_array_equal(one.coefficients, twin.coefficients)
    assert one.coefficients.dtype == np.complex128
    again = one.coherence(window=128)                # ... and after the result has been brought over
    np.testing.assert_array_equal(first.cross, again.cross)
    np.testing.assert_array_equal(one.fetch(), twin.fetch())


# -- 5. the error surface on the device --------------------------------------------------------------------------------
def test_error_surface_on_the_device():
    from ghost_amd.synthetic import lfp
    from ghost_amd.wave import ContinuousWaveletTransform
    x = lfp(4, 8192, FS, seed=1)
    kw = dict(fs=FS, freq_limits=[8, 200], voices_per_octave=4)
    cwt = ContinuousWaveletTransform()
    cwt.transform(x, multichannel=True, **kw)                                     # amplitude
    with pytest.raises(ValueError, match="complex"):
        cwt.coherence(window=64)
    cwt = ContinuousWaveletTransform()
    cwt.transform(x[0], output="complex", **kw)                                   # one channel, the reference's call
    with pytest.raises(ValueError, match="multichannel"):
        cwt.coherence(window=64)
    cwt.transform(x[:1], multichannel=True, output="complex", **kw)               # one channel of a multichannel call
    with pytest.raises(ValueError, match="2 channels"):
        cwt.coherence(window=64)
    cwt = ContinuousWaveletTransform()
    cwt.transform(x, multichannel=True, output="complex", devices=[0, 0], **kw)   # sharded
    with pytest.raises(ValueError, match="devices"):
        cwt.coherence(window=64)
    cwt = ContinuousWaveletTransform()
    cwt.transform(x, multichannel=True, output="complex", **kw)
    with pytest.raises(ValueError, match="window"):
        cwt.coherence(window=1)
    with pytest.raises(ValueError, match="outside"):
        cwt.coherence([[0, 4]], window=64)
    with pytest.raises(ValueError):
        cwt.coherence([[0, 1]], seed=0, window=64)
    with pytest.raises(ValueError):
        cwt.coherence([[2, 2]], window=64)
    assert cwt.coherence([[0, 3]], window=64).coherence.shape == (1, cwt.frequencies.size, 128)


# -- 6. a shape that exercises the tiles -------------------------------------------------------------------------------
def test_thirty_two_channels_all_pairs():
    from ghost_amd.synthetic import lfp
    c, n, window = 32, 1 << 18, 1000
    x = lfp(c, n, FS, seed=21)
    plan, result = _resident(x, np.geomspace(200.0, 2.0, 40))
    pairs = cm.all_pairs(c)
    assert len(pairs) == 496
    got = _run(result, pairs, window)
    n_bins = -(-n // window)
    assert got["coherence"].shape == (496, 40, n_bins) and got["power"].shape == (32, 40, n_bins)
    rng = np.random.default_rng(6)
    bound, worst = cm.gamma_bound(window), 0.0
    cells = [(int(rng.integers(496)), int(rng.integers(40)), int(rng.integers(n_bins))) for _ in range(198)]
    cells += [(0, 0, n_bins - 1), (495, 39, n_bins - 1)]                          # the short last bin
    for p, s, m in cells:
        a, b = pairs[p]
        w = result.to_host(np.complex64, scales=s, start=m * window, stop=(m + 1) * window)[:, 0]
        ref = cm.model(w[[a, b], None, :], [[0, 1]], window)
        assert ref["counts"].tolist() == [min(window, n - m * window)]
        g_dev = cm.gamma_of(got["cross"][p, s, m].reshape(1, 1, 1), got["power"][[a, b], s, m].reshape(2, 1, 1), [[0, 1]])
        err = abs(g_dev[0, 0, 0] - ref["gamma"][0, 0, 0])
        worst = max(worst, err)
        assert err <= bound, (p, s, m, err, bound)
        assert abs(float(got["coherence"][p, s, m]) - ref["coherence"][0, 0, 0]) <= 2 * bound
        for k, ch in enumerate((a, b)):
            assert abs(float(got["power"][ch, s, m]) - ref["power"][k, 0, 0]) <= cm.power_bound(window) * ref["power"][k, 0, 0]
    print("32 channels, 496 pairs: worst |gamma_dev - gamma_ref| %.3g (bound %.3g)" % (worst, bound))
    result.free()
    plan.close()
