"""output_stride=K on the MI355X: the strided result is the full-rate result's [..., ::K] -- bit for bit on the direct,
block-convolution and full-band scales (the same kernels, only fewer stores) and on every complex row; amplitude /
power rows of the k_synth7 levels within 5e-7 of a row's peak (the complex values k_synth7s makes are k_synth7's bit for
bit, but in the |.| instantiations the compiler contracts the last radix-16 layer's multiply-adds differently in the two
kernels: a last bit now and then) -- and it meets the reference on the goldens (gcwt_plan_set_output_stride)."""
import numpy as np
import pytest

from conftest import rel_err
from oracle import ghost_oracle as orc

pytestmark = pytest.mark.gpu

TOL = 1e-5
STRIDES = [2, 3, 4, 7, 16, 30, 32, 256, 1000]


SPECTRAL_TOL = 5e-7


def _same(plan, got, want, msg=""):
    """got == want on the rows of the direct / block-convolution / full-band scales and on every complex row, within
    SPECTRAL_TOL of the row's peak on the amplitude / power rows of the spectral scales."""
    from ghost_amd import _lib
    spectral = plan.scale_info()["method"] == _lib.SCALE_SPECTRAL
    if np.iscomplexobj(got):
        spectral[:] = False
    assert got.shape == want.shape, msg
    np.testing.assert_array_equal(got[:, ~spectral], want[:, ~spectral], err_msg=msg)
    if spectral.any():
        err = rel_err(got[:, spectral], want[:, spectral])
        assert err.max() <= SPECTRAL_TOL, (msg, err.max())


def _pair(x, fs, f, k, **kw):
    from ghost_amd.engine import CwtPlan
    x = np.atleast_2d(np.asarray(x, dtype=np.float32))
    full = CwtPlan(x.shape[1], x.shape[0], fs, f, **kw)
    strided = CwtPlan(x.shape[1], x.shape[0], fs, f, output_stride=k, **kw)
    return full, strided, full.execute(x), strided.execute(x)


def _methods(p):
    from ghost_amd import _lib
    m = p.scale_info()["method"]
    return {"interp": p.info["n_interp"] > 0,
            "spectral": (m == _lib.SCALE_SPECTRAL).sum() > p.info["n_interp"],
            "direct": (m == _lib.SCALE_DIRECT).any(),
            "exact": ((m == _lib.SCALE_BLOCKCONV) | (m == _lib.SCALE_FULLBAND)).any()}


@pytest.mark.parametrize("output", ["amplitude", "power", "complex"])
def test_strided_result_is_the_full_result_sliced(golden, output):
    """Every K, every output mode, on plans that exercise the interpolating and the 16/32-column spectral kernels
    (LFP at 1 kHz, 200 .. 2 Hz), the direct path (G11's heavy tails) and the block convolution / full band (G15's)."""
    from ghost_amd.synthetic import lfp
    seen = {"interp": False, "spectral": False, "direct": False, "exact": False}
    x = lfp(2, 60001, 1000.0, seed=7)
    g11, g15 = golden("g11_gamma_beta.npz"), golden("g15_blockconv.npz")
    cases = [(x, 1000.0, np.geomspace(200.0, 2.0, 24), {}),
             (g11["x"], float(g11["fs"]), g11["frequencies"], dict(gamma=3.0, beta=4.0)),
             (g11["x"], float(g11["fs"]), g11["frequencies"], dict(gamma=1.0, beta=5.0)),
             (g15["x"], float(g15["fs"]), g15["frequencies"], dict(gamma=3.0, beta=2.0, epoch_bounds=g15["epochs"]))]
    for xs, fs, f, kw in cases:
        for k in STRIDES:
            full, strided, a, b = _pair(xs, fs, f, k, output=output, **kw)
            for key, v in _methods(strided).items():
                seen[key] = seen[key] or v
            _same(strided, b, a[..., ::k], "K=%d %s" % (k, kw))
            full.close(); strided.close()
    if output == "complex":
        seen["interp"] = True                         # (the interpolating kernel makes amplitude / power only)
    assert all(seen.values()), seen


def test_goldens_sliced_meet_the_reference(golden):
    """G1, G5 (two epochs with a gap; K divides neither epoch start), G11 and G15 against the reference's columns
    that K keeps; columns in the epoch gap are exactly 0."""
    from ghost_amd.engine import CwtPlan
    from ghost_amd.wave import ContinuousWaveletTransform
    g = golden("g1_config1.npz")
    for k in (2, 3, 8):
        cwt = ContinuousWaveletTransform()
        cwt.transform(g["x"], fs=1000.0, freq_limits=[5, 200], voices_per_octave=6, output="complex", output_stride=k)
        cols = g["cols"][g["cols"] % k == 0]
        assert cols.size > 10
        assert rel_err(cwt.coefficients[:, cols // k], g["complex_cols"][:, g["cols"] % k == 0]).max() < TOL
    g = golden("g5_two_epochs.npz")
    for k in (7, 9):                                  # K divides neither epoch's first sample (6000)
        assert all(s % k for s in g["epoch_bounds"][:, 0] if s)
        cwt = ContinuousWaveletTransform()
        cwt.transform(g["x"], fs=float(g["fs"]), timestamps=g["timestamps"], output="complex", output_stride=k)
        c = cwt.coefficients
        assert c.shape[-1] == -(-g["x"].size // k) and cwt.time.size == c.shape[-1]
        np.testing.assert_array_equal(cwt.time, np.asarray(g["timestamps"])[::k])
        keep = g["cols"] % k == 0
        assert rel_err(c[:, g["cols"][keep] // k], g["complex_cols"][:, keep]).max() < TOL
        # samples outside every epoch: a gap [5990, 6013) cut out of the same recording
        eb = np.array([[0, 5990], [6013, 10000]])
        p = CwtPlan(g["x"].size, 1, float(g["fs"]), g["frequencies"], epoch_bounds=eb, output="complex",
                    output_stride=k)
        c = p.execute(g["x"][None])[0]
        gap = np.arange(-(-5990 // k), -(-6013 // k))
        assert gap.size > 0 and not np.any(c[:, gap]) and np.all(np.any(c[:, gap[-1] + 1:], axis=1))
    g = golden("g11_gamma_beta.npz")
    for gamma, beta in ((3, 8), (3, 4), (1, 5)):
        tag = "g%d_b%d" % (gamma, beta)
        p = CwtPlan(g["x"].size, 1, float(g["fs"]), g["frequencies"], output="complex", gamma=gamma, beta=beta,
                    output_stride=4)
        c = p.execute(g["x"][None])[0]
        keep = g["cols"] % 4 == 0
        assert rel_err(c[:, g["cols"][keep] // 4], g["complex_cols_" + tag][:, keep]).max() < TOL, tag
    g = golden("g15_blockconv.npz")
    for gamma, beta in g["pairs"]:
        tag = "%g_%g" % (gamma, beta)
        p = CwtPlan(g["x"].size, 1, float(g["fs"]), g["frequencies"], gamma=float(gamma), beta=float(beta),
                    epoch_bounds=g["epochs"], output="complex", output_stride=5)
        c = p.execute(g["x"][None])[0]
        keep = g["cols"] % 5 == 0
        err = np.abs(c[:, g["cols"][keep] // 5] - g["complex_cols_" + tag][:, keep]).max(axis=1) / g["rowmax_" + tag]
        assert err.max() < TOL, (tag, err)


def test_time_blocks_and_streaming():
    """Epochs cut into time blocks (max_fft_log2=13) map each block's kept samples to columns by the recording's
    sample index; execute_block at an unaligned start returns exactly the kept columns of its range."""
    from ghost_amd.synthetic import lfp
    fs, n = 1000.0, 30000
    x = lfp(2, n, fs) + 0.75
    f = [300.0, 150.0, 40.0, 12.0]
    for k in (3, 32, 1000):
        full, p, a, b = _pair(x, fs, f, k, output="amplitude", max_fft_log2=13)
        assert len(p.segments()) > 2
        _same(p, b, a[..., ::k], "K=%d" % k)
        for start, length in ((7777, 9001), (1, 2), (k + 1, k - 1), (n - 5, 5)):
            blk = p.execute_block(x, start, length)
            c0, c1 = -(-start // k), -(-(start + length) // k)
            assert blk.shape[-1] == c1 - c0, (k, start, length)
            np.testing.assert_array_equal(blk, b[..., c0:c1])
    full, p, a, b = _pair(x, fs, f, 5, output="complex")
    np.testing.assert_array_equal(p.execute_block(x, 101, 5000), b[..., 21:1021])
    _same(p, b, a[..., ::5])


def test_auto_precision_under_a_mains_line_reroutes_into_the_strided_rows():
    """precision='auto' with a 60 Hz line 300 x the recording's spread inside the band: the same scales are rerouted
    to the exact paths as at K = 1, and their strided rows are the full-rate rerouted rows sliced."""
    from ghost_amd.engine import CwtPlan
    from ghost_amd.synthetic import lfp_channel
    fs, n = 1000.0, 250000
    f = np.geomspace(200.0, 2.0, 100)
    t = np.arange(n) / fs
    base = lfp_channel(n, fs, 3).astype(np.float64)
    win = np.sin(np.pi * np.arange(n) / n) ** 2
    x = (base + 300.0 * base.std() * win * np.sin(2 * np.pi * 60.0 * t)).astype(np.float32)
    full = CwtPlan(n, 1, fs, f, output="amplitude")
    a = full.execute(x[None])
    r1 = full.precision_report()
    assert r1["rerouted"] > 0
    for k in (4, 30):
        p = CwtPlan(n, 1, fs, f, output="amplitude", output_stride=k)
        b = p.execute(x[None])
        assert p.precision_report()["rerouted"] == r1["rerouted"]
        _same(p, b, a[..., ::k], "K=%d" % k)
        over = np.argsort(p.precision_report()["predicted"])[-r1["rerouted"]:]   # the rerouted rows: exact paths, bit-equal
        np.testing.assert_array_equal(b[:, over], a[:, over, ::k])
    ref = orc.cwt_amplitude(x.astype(np.float64), fs, f[[10, 60]])
    assert rel_err(b[0][[10, 60]], ref[:, ::30]).max() < TOL


def test_public_surface():
    """Shapes of amplitude / power / coefficients / time, fetch() in columns, lazy=False, devices=[0, 0], a
    device-resident plan with a row pitch, and a resident buffer ~1/K of the full one."""
    from ghost_amd import _lib
    from ghost_amd.engine import CwtPlan, DeviceBuffer
    from ghost_amd.synthetic import lfp
    from ghost_amd.wave import ContinuousWaveletTransform
    fs, n, k = 1000.0, 20011, 7
    x = lfp(3, n, fs, seed=3)
    ts = 12.5 + np.arange(n) / fs
    kinds = {"amplitude": "amplitude", "power": "power", "complex": "coefficients"}
    for output, attr in kinds.items():
        full = ContinuousWaveletTransform()
        full.transform(x, timestamps=ts, fs=fs, freq_limits=[4, 250], multichannel=True, output=output)
        want = getattr(full, attr)[..., ::k]
        for lazy in (True, False):
            cwt = ContinuousWaveletTransform()
            cwt.transform(x, timestamps=ts, fs=fs, freq_limits=[4, 250], multichannel=True, output=output,
                          output_stride=k, lazy=lazy)
            got = getattr(cwt, attr)
            assert got.shape == (3, full.frequencies.size, -(-n // k))
            np.testing.assert_allclose(cwt.time, ts[::k])
            assert rel_err(got, want).max() <= SPECTRAL_TOL
            part = cwt.fetch(slice(2, 5), 10, 100)
            np.testing.assert_array_equal(part, got[:, 2:5, 10:100])
    # devices=[0, 0]: two plans on one device, the same bits as one
    one, two = ContinuousWaveletTransform(), ContinuousWaveletTransform()
    one.transform(x, fs=fs, freq_limits=[4, 250], multichannel=True, output_stride=k)
    two.transform(x, fs=fs, freq_limits=[4, 250], multichannel=True, output_stride=k, devices=[0, 0])
    np.testing.assert_array_equal(one.amplitude, two.amplitude)
    # the resident buffer is 1/K of the full one (rows padded to 32 columns)
    f = full.frequencies
    pf, ps = CwtPlan(n, 3, fs, f), CwtPlan(n, 3, fs, f, output_stride=k)
    rf, rs = pf.execute_resident(x), ps.execute_resident(x)
    assert rs.nbytes == 3 * f.size * ((-(-n // k) + 31) & ~31) * 4 and rs.nbytes < rf.nbytes / (k - 1)
    _same(ps, rs.to_host(), rf.to_host()[..., ::k])
    # device in, device out, a row pitch in columns; the stride is fixed once the plan has run
    cols = -(-n // k)
    pitch = (cols + 31) & ~31
    xb = DeviceBuffer(4 * 3 * n)
    xb.upload(np.ascontiguousarray(x, dtype=np.float32))
    ob = DeviceBuffer(4 * 3 * f.size * pitch)
    ps.set_row_pitch(pitch)
    ps.execute_device(xb, ob)
    got = ob.download((3, f.size, pitch), np.float32)[..., :cols]
    np.testing.assert_array_equal(got, rs.to_host())
    assert _lib.lib.gcwt_plan_set_output_stride(ps._handle, 2) == _lib.ERR_INVALID
    for b in (xb, ob, rf, rs):
        b.free()


def test_headline_shape_at_stride_4():
    """128 ch x 1e6 samples x 100 scales, K = 4, resident: rows of channels {0, 7, 127} against the K = 1 result and
    against the oracle on one scale per decimation level."""
    from ghost_amd.engine import CwtPlan, DeviceBuffer
    from ghost_amd.synthetic import lfp
    fs, C, N, S, k = 1000.0, 128, 1000000, 100, 4
    f = np.geomspace(200.0, 2.0, S)
    base = lfp(8, N, fs, seed=1234)
    xbuf = DeviceBuffer(4 * C * N)
    for c in range(C):
        xbuf.upload(base[c % 8], offset_bytes=4 * c * N)
    plan = CwtPlan(N, C, fs, f, output="amplitude", output_stride=k)
    cols = N // k
    assert plan.info["out_bytes"] == 4 * C * S * cols
    dec = plan.scale_info()["decimation"]
    scales = sorted({int(np.flatnonzero(dec == r)[0]) for r in np.unique(dec)} | {57})
    obuf = DeviceBuffer(plan.info["out_bytes"])
    plan.execute_device(xbuf, obuf)
    rows = {(c, s): obuf.download((cols,), np.float32, offset_bytes=4 * (c * S + s) * cols)
            for c in (0, 7, 127) for s in scales}
    obuf.free()
    plan.close()
    full = CwtPlan(N, C, fs, f, output="amplitude")
    fbuf = DeviceBuffer(full.info["out_bytes"])
    full.execute_device(xbuf, fbuf)
    for (c, s), row in rows.items():
        want = fbuf.download((N,), np.float32, offset_bytes=4 * (c * S + s) * N)[::k]
        assert rel_err(row, want) <= SPECTRAL_TOL, (c, s)
    fbuf.free()
    xbuf.free()
    for c in (0,):
        ref = orc.cwt_amplitude(base[c % 8].astype(np.float64), fs, f[scales])
        for i, s in enumerate(scales):
            assert rel_err(rows[(c, s)], ref[i][::k]) < TOL, (c, s)
