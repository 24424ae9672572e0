"""The operator layer (ghost_amd/sigtools: ConvPlan, fastconv_*, chirpz_*, analytic_signal_*; conv_plan.cpp,
conv_kernels.hip, spectral_ops.cpp, ops64.hip) at every column-FFT length, chunk edge, length edge and admitted limit.
The shapes and the classes they stand for are in sigtools_cases.py (held to the code's arithmetic by
test_sigtools_cases_cpu.py); here the device first confirms the geometry (ConvPlan.fft_length / .chunk / .n_chunks),
then its numbers meet a host reference one step above it in precision:

  float32 operators   NumPy / SciPy in float64 on the float32-rounded inputs; the suite's gates: convolution and
                      analytic signal 1e-5 x the result's peak, DFT 3e-6 x peak
  float64 operators   scipy.fft / a direct sum on np.longdouble (80-bit, eps 1.1e-19) rounded to float64; np.allclose at
                      its defaults, and rtol 1e-9 / atol 1e-12 x peak on the chunked convolution.  The error against the
                      peak is printed beside 64 eps log2(L), what float64 transforms should stay well under (allclose
                      at its defaults would let float32 arithmetic through); it is a figure to read, not yet a gate.

Every figure is printed before it is asserted (pytest -s shows them).

Which test catches which break (each was read against the code, k = the first case that fails):
  chunk0 in k_conv_store ignored               test_chunk_geometry[52345-1] (chunk 16 lands on chunk 0) and [100000-3]
  the (total - count) / 2 crop off by one      test_same_crop_element_by_element, test_length_edges (every pair)
  P1 == 256 / 512 complex-forward dispatch     test_dft_every_p1[256], [512]; test_conv_every_p1[256], [512]
  the radix-2 first stage of fft64             test_dft64_powers_of_two (2, 8, 32, ... every odd log2), test_dft64_bluestein
  the pow2 switch of dft_f64                   a non-power of two sent to the direct path: test_dft64_bluestein at 2^k -+ 1
                                               (L < n); a power of two sent through Bluestein is still a correct DFT, so
                                               test_dft64_powers_of_two holds the impulse's transform to exact ones, which
                                               only the direct path gives
"""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.fft as sfft
from scipy.signal import convolve, fftconvolve, hilbert

import sigtools_cases as sc

pytestmark = pytest.mark.gpu

LD, CLD = np.longdouble, np.clongdouble
EPS64 = float(np.finfo(np.float64).eps)
CONV_TOL, DFT_TOL, ANALYTIC_TOL = 1e-5, 3e-6, 1e-5


def _rel(got, ref):
    peak = np.abs(ref).max()
    return float(np.abs(got - ref).max() / (peak if peak > 0 else 1.0))


def _gate32(got, ref, tol, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    e = _rel(got, ref)
    print("%-60s err/peak %.3g (gate %.3g)" % (what, e, tol))
    assert e <= tol, (what, e)


def _gate64(got, ref_ld, lg, what, chunked=False):
    """float64 result against the longdouble reference rounded to float64."""
    assert np.finfo(LD).eps < 2e-19                    # the reference is a real step above float64
    ref = ref_ld.astype(np.complex128 if np.iscomplexobj(ref_ld) else np.float64)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    e, bound = _rel(got, ref), 64 * EPS64 * max(1, lg)
    print("%-60s err/peak %.3g (64 eps log2 L = %.3g)" % (what, e, bound))
    assert np.allclose(got, ref), what
    if chunked:
        assert np.allclose(got, ref, rtol=1e-9, atol=1e-12 * np.abs(ref).max()), what


def _crop(full, n, m, mode):
    """convolution.py:79-87 of the reference."""
    count = {"full": n + m - 1, "same": n, "valid": n - m + 1}[mode]
    first = (n + m - 1 - count) // 2
    return full[first:first + count]


def _modes(n, m):
    return [mode for mode in sc.MODES if mode != "valid" or n >= m]


def _signal32(rng, shape):
    """standard_normal rounded to float32: the reference sees the numbers the device sees."""
    return rng.standard_normal(shape).astype(np.float32)


def _kernel32(rng, m, complex_=True):
    k = rng.standard_normal(m)
    return (k + 1j * rng.standard_normal(m)).astype(np.complex64) if complex_ else k.astype(np.float32)


def _full_ld(x, k):
    """The full linear convolution in longdouble: a direct sum where it is small, scipy.fft on the padded pair beyond."""
    cplx = np.iscomplexobj(x) or np.iscomplexobj(k)
    xl, kl = x.astype(CLD if np.iscomplexobj(x) else LD), k.astype(CLD if np.iscomplexobj(k) else LD)
    n, m = len(x), len(k)
    if n * m <= 4_000_000:
        return np.convolve(xl, kl)
    L = sfft.next_fast_len(n + m - 1, real=not cplx)
    if cplx:
        return sfft.ifft(sfft.fft(xl, L) * sfft.fft(kl, L))[:n + m - 1]
    return sfft.irfft(sfft.rfft(xl, L) * sfft.rfft(kl, L), L)[:n + m - 1]


def _plan_create_rc(n, m, channels, fft_log2):
    """The C entry point itself: (return code, message)."""
    import ghost_amd.sigtools                          # noqa: F401  (declares the entry point's arguments)
    from ghost_amd._lib import lib
    h = C.c_void_p()
    rc = lib.gcwt_conv_plan_create(C.byref(h), n, m, channels, fft_log2, -1)
    msg = lib.gcwt_last_error().decode("utf-8", "replace") if rc else ""
    if h:
        lib.gcwt_conv_plan_destroy(h)
    return rc, msg


# ---- A. every P1 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p1,n,m", sc.A_CONV)
def test_conv_every_p1(p1, n, m):
    """One two-channel convolution per column length (real forward, complex forward of the kernel, inverse), and the
    bit-level properties at that length: a slot is transformed on its own, so channel c of the batch is the one-channel
    plan on that row; two executes of one plan agree."""
    from ghost_amd.sigtools import ConvPlan
    rng = np.random.default_rng(1000 + p1)
    x, k = _signal32(rng, (sc.A_CONV_C, n)), _kernel32(rng, m)
    g = sc.conv_geometry(n, m, None, sc.A_CONV_C)
    plan = ConvPlan(n, m, sc.A_CONV_C)
    assert (plan.fft_length, plan.chunk, plan.n_chunks) == (p1 * 4096, g["step"], 1) and g["P1"] == p1
    got = plan.set_kernel(k).execute(x)
    assert got.dtype == np.complex64
    for c in range(sc.A_CONV_C):
        _gate32(got[c], fftconvolve(x[c].astype(np.float64), k.astype(np.complex128), mode="same"), CONV_TOL,
                "conv P1=%d n=%d m=%d ch %d" % (p1, n, m, c))
    np.testing.assert_array_equal(plan.execute(x), got)
    one = ConvPlan(n, m, 1)
    assert (one.fft_length, one.chunk, one.n_chunks) == (plan.fft_length, plan.chunk, 1)
    np.testing.assert_array_equal(one.set_kernel(k).execute(x[1]), got[1])
    plan.close()
    one.close()


@functools.lru_cache(maxsize=None)
def _dft_case(p1, n, real):
    rng = np.random.default_rng(2000 + p1 + (500 if real else 0))
    z = _signal32(rng, n) if real else (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    z.setflags(write=False)
    return z


def _host_single(z, inverse):
    """What a plain single-precision transform of the same input makes on the host (the yardstick of the issue)."""
    f = sfft.ifft if inverse else sfft.fft
    got = f(z.astype(np.complex64))
    assert got.dtype == np.complex64
    return got


@pytest.mark.parametrize("p1,n", sc.A_DFT)
def test_dft_every_p1(p1, n):
    """Forward and inverse chirp-z DFT of complex input with 2 n - 1 in (P / 2, P]: the complex forward and the inverse
    column pass at every P1 (k_fft_cols256<-1, false> at 256, k_fft_colsq<-1, false, 1|2> at 512 and 1024).
    P1 = 1024 is n = 2^21, the largest length admitted."""
    from ghost_amd.sigtools import chirpz_dft_hip, chirpz_idft_hip
    assert sc.chirp_geometry(n)["P1"] == p1
    z = _dft_case(p1, n, False)
    z64 = z.astype(np.complex128)
    for inverse, fn, host in ((False, chirpz_dft_hip, np.fft.fft), (True, chirpz_idft_hip, np.fft.ifft)):
        ref = host(z64)
        got = fn(z)
        assert got.dtype == np.complex64
        if p1 >= 256:
            print("    host complex64 transform, n=%d inverse=%d: err/peak %.3g" % (n, inverse, _rel(_host_single(z, inverse), ref)))
        _gate32(got, ref, DFT_TOL, "dft P1=%d n=%d inverse=%d" % (p1, n, inverse))


@pytest.mark.parametrize("p1", sc.A_DFT_REAL)
def test_dft_real_input(p1):
    from ghost_amd.sigtools import chirpz_dft_hip, chirpz_idft_hip
    n = dict(sc.A_DFT)[p1]
    x = _dft_case(p1, n, True)
    x64 = x.astype(np.float64)
    print("    host complex64 transform, n=%d: err/peak %.3g" % (n, _rel(_host_single(x, False), np.fft.fft(x64))))
    _gate32(chirpz_dft_hip(x), np.fft.fft(x64), DFT_TOL, "dft real P1=%d n=%d" % (p1, n))
    _gate32(chirpz_idft_hip(x), np.fft.ifft(x64), DFT_TOL, "idft real P1=%d n=%d" % (p1, n))


@pytest.mark.parametrize("p1,n,f", sc.A_ANALYTIC)
def test_analytic_signal_p1(p1, n, f):
    from ghost_amd.sigtools import analytic_signal_hip
    assert sc.chirp_geometry(f or n)["P1"] == p1
    x = _signal32(np.random.default_rng(3000 + p1), n)
    ref = hilbert(x.astype(np.float64), N=f)[:n]
    got = analytic_signal_hip(x, fft_length=f)
    assert got.dtype == np.complex64
    _gate32(got, ref, ANALYTIC_TOL, "analytic P1=%d n=%d fft_length=%s" % (p1, n, f))


# ---- B. chunk geometry -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _chunk_case(n, C_):
    rng = np.random.default_rng(4000 + n % 1000 + C_)
    x, k = _signal32(rng, (C_, n)), _kernel32(rng, sc.B_M)
    full = np.stack([fftconvolve(x[c].astype(np.float64), k.astype(np.complex128), mode="full") for c in range(C_)])
    for a in (x, k, full):
        a.setflags(write=False)
    return x, k, full


@pytest.mark.parametrize("n,C_,n_chunks,n_batches,last_batch,last_samples", sc.B_CHUNK)
def test_chunk_geometry(n, C_, n_chunks, n_batches, last_batch, last_samples):
    """fft_length 4096, 777 taps: exactly one full batch; a second batch of one chunk that holds one real sample; two
    batches of 16 + 15 chunks of three channels.  Every mode, every channel, every sample."""
    from ghost_amd.sigtools import ConvPlan, fastconv_hip
    m = sc.B_M
    x, k, full = _chunk_case(n, C_)
    g = sc.conv_geometry(n, m, sc.B_FFT, C_)
    assert (g["n_chunks"], g["n_batches"], g["last_batch"]) == (n_chunks, n_batches, last_batch)
    plan = ConvPlan(n, m, C_, fft_length=sc.B_FFT).set_kernel(k)
    assert (plan.fft_length, plan.chunk, plan.n_chunks) == (4096, 3320, n_chunks)
    for mode in sc.MODES:
        got = plan.execute(x, mode=mode)
        for c in range(C_):
            _gate32(got[c], _crop(full[c], n, m, mode), CONV_TOL, "chunks n=%d C=%d %s ch %d" % (n, C_, mode, c))
        if C_ == 1:
            np.testing.assert_array_equal(fastconv_hip(x[0], k, mode=mode, fft_length=sc.B_FFT), got[0])
    plan.close()


def test_chunked_batches_bit_properties():
    """The 31-chunk, three-channel plan: device-resident execution gives the bits of execute(); channel c is the
    one-channel plan of the same n, m, fft_length on that row; a second set_kernel on a used plan gives the bits of a
    fresh plan."""
    from ghost_amd.engine import DeviceBuffer
    from ghost_amd.sigtools import ConvPlan
    n, C_, m = sc.B_CHUNK[2][0], sc.B_CHUNK[2][1], sc.B_M
    x, k, _ = _chunk_case(n, C_)
    plan = ConvPlan(n, m, C_, fft_length=sc.B_FFT).set_kernel(k)
    assert plan.n_chunks == 31
    for mode in ("same", "full"):
        host = plan.execute(x, mode=mode)
        count = plan.count(mode)
        xb, ob = DeviceBuffer(4 * C_ * n), DeviceBuffer(8 * C_ * count)
        xb.upload(x)
        ob.zero()
        plan.execute_device(xb, ob, mode=mode)
        np.testing.assert_array_equal(ob.download((C_, count), np.complex64), host)
        np.testing.assert_array_equal(plan.execute(x, mode=mode), host)
        xb.free()
        ob.free()
    host = plan.execute(x)
    one = ConvPlan(n, m, 1, fft_length=sc.B_FFT).set_kernel(k)
    assert (one.fft_length, one.chunk, one.n_chunks) == (plan.fft_length, plan.chunk, plan.n_chunks)
    for c in range(C_):
        np.testing.assert_array_equal(one.execute(x[c]), host[c])
    k2 = _kernel32(np.random.default_rng(4999), m, complex_=False)
    used = plan.set_kernel(k2).execute(x)
    fresh = ConvPlan(n, m, C_, fft_length=sc.B_FFT).set_kernel(k2).execute(x)
    assert used.dtype == np.float32
    np.testing.assert_array_equal(used, fresh)
    _gate32(used[2], fftconvolve(x[2].astype(np.float64), k2.astype(np.float64), mode="same"), CONV_TOL, "second kernel")


def test_channel_cap():
    """C = 4095: one chunk, 4095 slots, every channel compared (one batched host FFT product); 4096 is refused."""
    from ghost_amd._lib import GhostCwtError, ERR_UNSUPPORTED
    from ghost_amd.sigtools import ConvPlan
    C_, n, m = sc.B_MANY["C"], sc.B_MANY["n"], sc.B_MANY["m"]
    rng = np.random.default_rng(4095)
    x, k = _signal32(rng, (C_, n)), _kernel32(rng, m)
    plan = ConvPlan(n, m, C_)
    assert (plan.fft_length, plan.n_chunks, plan.chunk) == (4096, 1, 4096 - (m - 1))
    full = np.fft.ifft(np.fft.fft(x.astype(np.float64), 2048, axis=1) * np.fft.fft(k.astype(np.complex128), 2048))[:, :n + m - 1]
    plan.set_kernel(k)
    for mode in sc.MODES:
        got = plan.execute(x, mode=mode)
        ref = np.stack([_crop(full[c], n, m, mode) for c in range(C_)])
        assert got.shape == ref.shape
        err = np.abs(got - ref).max(axis=1) / np.abs(ref).max(axis=1)
        print("C=4095 %s: worst channel %d err/peak %.3g" % (mode, err.argmax(), err.max()))
        assert (err <= CONV_TOL).all(), (mode, int(err.argmax()), float(err.max()))
    plan.close()
    with pytest.raises(GhostCwtError, match="more than 4095 channels") as exc:
        ConvPlan(n, m, C_ + 1)
    assert exc.value.code == ERR_UNSUPPORTED


def test_chunks_beyond_one_row():
    """fft_length 16384, 2000 taps, 120000 samples, two channels: 9 chunks at P1 = 4."""
    from ghost_amd.sigtools import ConvPlan
    w = sc.B_WIDE
    n, m, C_ = w["n"], w["m"], w["C"]
    rng = np.random.default_rng(16384)
    x, k = _signal32(rng, (C_, n)), _kernel32(rng, m)
    plan = ConvPlan(n, m, C_, fft_length=w["fft_length"]).set_kernel(k)
    assert (plan.fft_length, plan.chunk, plan.n_chunks) == (16384, 16384 - 1999, 9)
    full = [fftconvolve(x[c].astype(np.float64), k.astype(np.complex128), mode="full") for c in range(C_)]
    for mode in sc.MODES:
        got = plan.execute(x, mode=mode)
        for c in range(C_):
            _gate32(got[c], _crop(full[c], n, m, mode), CONV_TOL, "P1=4 chunks %s ch %d" % (mode, c))
    plan.close()


# ---- C. length edges -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", sc.C_EDGES)
def test_length_edges(n, m):
    """float32 and float64, real and complex kernels, every mode that is defined, against the direct longdouble sum."""
    from ghost.sigtools import fastconv_scipy
    from ghost_amd.sigtools import ConvPlan, fastconv_hip
    rng = np.random.default_rng(5000 + 13 * n + m)
    plan = ConvPlan(n, m)
    assert (plan.fft_length, plan.n_chunks, plan.chunk) == (4096, 1, 4096 - (m - 1))
    plan.close()
    for complex_ in (False, True):
        x, k = _signal32(rng, n), _kernel32(rng, m, complex_)
        x64, k64 = x.astype(np.float64), k.astype(np.complex128 if complex_ else np.float64)
        full = _full_ld(x64, k64)
        lg = sc.conv64_path(n, m)["lg"]
        for mode in _modes(n, m):
            ref = _crop(full, n, m, mode)
            what = "edge n=%d m=%d %s %s" % (n, m, "complex" if complex_ else "real", mode)
            got = fastconv_hip(x, k, mode=mode)
            assert got.dtype == (np.complex64 if complex_ else np.float32)
            _gate32(got, ref.astype(np.complex128 if complex_ else np.float64), CONV_TOL, what)
            _gate64(fastconv_hip(x64, k64, mode=mode, precision="high"), ref, lg, what + " high")
            _gate64(fastconv_scipy(x64, k64, mode=mode), ref, lg, what + " fastconv_scipy")
        if n < m:
            for fn, kw in ((fastconv_hip, {}), (fastconv_hip, {"precision": "high"}), (fastconv_scipy, {})):
                with pytest.raises(ValueError, match="Cannot do a 'valid' convolution because the input is shorter than the kernel"):
                    fn(x64, k64, mode="valid", **kw)


def test_same_crop_element_by_element():
    """An odd and an even kernel length side by side against scipy.signal.convolve(..., 'same'), element by element: the
    two crops differ by one sample, so a crop off by one fails one of them at every element."""
    from ghost_amd.sigtools import fastconv_hip
    rng = np.random.default_rng(5999)
    (n, m_odd), (_, m_even) = sc.C_SAME_PAIR
    x = _signal32(rng, n)
    for m in (m_odd, m_even):
        for complex_ in (False, True):
            k = _kernel32(rng, m, complex_)
            ref = convolve(x.astype(np.float64), k.astype(np.complex128 if complex_ else np.float64), mode="same")
            got = fastconv_hip(x, k, mode="same")
            assert got.shape == ref.shape
            assert (np.abs(got - ref) <= CONV_TOL * np.abs(ref).max()).all(), m
            hi = fastconv_hip(x.astype(np.float64), k.astype(ref.dtype), mode="same", precision="high")
            assert hi.dtype == ref.dtype and np.allclose(hi, ref), m
            # and the neighbouring crop is far away: the check can tell them apart
            assert np.abs(np.roll(ref, 1) - ref).max() > 0.1 * np.abs(ref).max()


@pytest.mark.parametrize("f,m,n,route", sc.C_FREQ)
def test_freq_domain_edges(f, m, n, route):
    """fastconv_freq_hip in float32 and 'high': DFTs of 4096 bins with 1, 2 and 4096 taps (step = 1: as one plan of 4096
    one-sample chunks when the signal is one sample, through the time domain when it is longer), and two grids the plan
    does not take (3000 and 2048 bins)."""
    from ghost_amd.sigtools import convolution, fastconv_freq_hip
    rng = np.random.default_rng(6000 + f + m + n)
    assert sc.freq_route(n, m, f) == route
    for complex_ in (False, True):
        x, k = _signal32(rng, n), _kernel32(rng, m, complex_)
        x64, k64 = x.astype(np.float64), k.astype(np.complex128 if complex_ else np.float64)
        Y = sfft.fft(k64, f)
        full = _full_ld(x64, k64)
        for mode in _modes(n, m):
            ref = _crop(full, n, m, mode).astype(np.complex128 if complex_ else np.float64)
            what = "freq f=%d m=%d n=%d %s %s" % (f, m, n, "complex" if complex_ else "real", mode)
            got = fastconv_freq_hip(x, Y, m, mode=mode)
            assert got.dtype == (np.complex64 if complex_ else np.float32), what
            _gate32(got, ref, CONV_TOL, what)
            hi = fastconv_freq_hip(x64, Y, m, mode=mode, precision="high")
            assert hi.shape == ref.shape and hi.dtype == ref.dtype, what
            print("%-60s err/peak %.3g" % (what + " high", _rel(hi, ref)))
            assert np.allclose(hi, ref), what
        # the route taken, from the plan the call left behind
        key = (n, m, f if route == "plan" else None, -1)
        assert key in convolution._cache, (key, list(convolution._cache))
        g = sc.conv_geometry(n, m, f if route == "plan" else None)
        plan = convolution._cache[key]
        assert (plan.fft_length, plan.chunk, plan.n_chunks) == (g["P"], g["step"], g["n_chunks"])


# ---- D. float64 ------------------------------------------------------------------------------------------------------------
def _dft64_check(n, seed):
    from ghost.sigtools import chirpz_dft
    from ghost_amd.sigtools import chirpz_dft_hip, chirpz_idft_hip
    rng = np.random.default_rng(seed)
    lg = sc.dft64_path(n)["lg"]
    for real in (True, False):
        z = rng.standard_normal(n) if real else rng.standard_normal(n) + 1j * rng.standard_normal(n)
        zl = z.astype(LD if real else CLD)
        what = "dft64 n=%d (%s, lg %d) %s" % (n, sc.dft64_path(n)["path"], lg, "real" if real else "complex")
        _gate64(chirpz_dft_hip(z, precision="high"), sfft.fft(zl), lg, what)
        _gate64(chirpz_idft_hip(z, precision="high"), sfft.ifft(zl), lg, what + " inverse")
        if real:
            np.testing.assert_array_equal(chirpz_dft(z), chirpz_dft_hip(z, precision="high"))


def test_dft64_powers_of_two():
    """Every power of two from 1 to 2^12 -- log2 L odd and even from the shortest length up, so the radix-2 first stage
    and phase64's shift at their smallest -- forward and inverse, real and complex input."""
    from ghost_amd.sigtools import chirpz_dft_hip
    for n in sc.D_POW2:
        if n <= 1 << 12:
            assert sc.dft64_path(n)["path"] == "direct"
            _dft64_check(n, 7000 + n)
            # the direct path adds and copies an impulse's ones and never rounds; Bluestein makes them by three
            # transforms and cannot: this is what pins the pow2 switch of dft_f64
            delta = np.zeros(n)
            delta[0] = 1.0
            np.testing.assert_array_equal(chirpz_dft_hip(delta, precision="high"), np.ones(n, dtype=np.complex128))


@pytest.mark.parametrize("n", [n for n in sc.D_POW2 if n > 1 << 12])
def test_dft64_large_powers_of_two(n):
    _dft64_check(n, 7000 + n % 997)


def test_dft64_bluestein():
    """Bluestein from 3 points up, on both sides of 2^5, 2^11 and 2^16 (the direct / Bluestein switch: the power of two
    between each pair is in the tests above), a round and a prime length."""
    for n in sc.D_BLUESTEIN:
        if n < 1 << 20:
            assert sc.dft64_path(n)["path"] == "bluestein"
            _dft64_check(n, 8000 + n % 997)


def test_dft64_bluestein_on_2_24():
    """3 x 2^21 points: Bluestein on L = 2^24, the largest transform fft64 makes."""
    from ghost_amd.sigtools import chirpz_dft_hip
    n = 3 << 21
    assert sc.dft64_path(n) == {"path": "bluestein", "lg": 24, "L": 1 << 24, "radix2": False}
    rng = np.random.default_rng(8024)
    z = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    _gate64(chirpz_dft_hip(z, precision="high"), sfft.fft(z.astype(CLD)), 24, "dft64 n=3*2^21")


def test_analytic_signal64():
    from ghost.sigtools import analytic_signal_fftw
    from ghost_amd.sigtools import analytic_signal_hip
    rng = np.random.default_rng(9000)
    for n, f in sc.D_ANALYTIC:
        x = rng.standard_normal(n)
        F = n if f is None else f
        xl = np.zeros(F, dtype=LD)
        xl[:n] = x
        h = np.zeros(F, dtype=LD)
        h[0] = 1
        h[1:(F + 1) // 2] = 2
        if F % 2 == 0:
            h[F // 2] = 1
        ref = sfft.ifft(sfft.fft(xl) * h)[:n]
        got = analytic_signal_hip(x, fft_length=f, precision="high")
        _gate64(got, ref, sc.dft64_path(F)["lg"], "analytic64 n=%d fft_length=%s" % (n, f))
        assert np.allclose(got, hilbert(x, N=f)[:n])
        np.testing.assert_array_equal(analytic_signal_fftw(x, fft_length=f), got)


@pytest.mark.parametrize("n,m", sc.D_CONV_EXACT)
def test_fastconv64_at_a_power_of_two(n, m):
    """n + m - 1 = 2^12 exactly (L = 2^12, no padding at all) and 2^12 + 1 (L = 2^13)."""
    from ghost_amd.sigtools import fastconv_hip
    p = sc.conv64_path(n, m)
    assert p["L"] == (4096 if n + m - 1 == 4096 else 8192)
    rng = np.random.default_rng(9100 + n)
    x, k = rng.standard_normal(n), rng.standard_normal(m) + 1j * rng.standard_normal(m)
    full = _full_ld(x, k)
    for mode in sc.MODES:
        _gate64(fastconv_hip(x, k, mode=mode, precision="high"), _crop(full, n, m, mode), p["lg"], "conv64 total=%d %s" % (n + m - 1, mode))


def test_fastconv64_chunked_lg23():
    """2^24 samples with a Hann-tapered real kernel of 2^20 + 3 taps, 'same': overlap-add chunks of 2^23 points
    (lg = ilog2(4 m) = 23 > 22, a radix-2 first stage), three of them."""
    from ghost_amd.sigtools import fastconv_hip
    c = sc.D_CHUNKED
    n, m = c["n"], c["m"]
    p = sc.conv64_path(n, m)
    assert (p["path"], p["lg"], p["n_chunks"]) == ("chunked", 23, 3)
    rng = np.random.default_rng(9223)
    x, k = rng.standard_normal(n), rng.standard_normal(m) * np.hanning(m)
    L = 9 << 21                                             # >= n + m - 1, smooth for the host
    assert L >= n + m - 1
    ref = sfft.irfft(sfft.rfft(x.astype(LD), L) * sfft.rfft(k.astype(LD), L), L)
    assert ref.dtype == LD
    ref = _crop(ref[:n + m - 1], n, m, "same")
    got = fastconv_hip(x, k, mode="same", precision="high")
    _gate64(got, ref, 23, "conv64 chunked lg=23", chunked=True)


# ---- F. grids the C entry point refuses --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,f,taken", sc.F_REFUSED)
def test_long_kernel_on_a_short_grid(n, m, f, taken):
    """fft_length = 4096 with 3700 and with 4096 taps (step = 1): the reference takes any fft_length >= m and the result
    does not depend on it, so the Python layer takes the next grid the plan admits; the C entry point still refuses."""
    from ghost_amd._lib import ERR_UNSUPPORTED
    from ghost_amd.sigtools import ConvPlan, fastconv_hip, fastconv_freq_hip
    rc, msg = _plan_create_rc(n, m, 1, sc.ceil_log2(f))
    assert rc == ERR_UNSUPPORTED and "kernel too long for overlap-save chunks" in msg
    plan = ConvPlan(n, m, fft_length=f)
    g = sc.conv_geometry(n, m, f)
    assert (plan.fft_length, plan.chunk, plan.n_chunks) == (taken, g["step"], g["n_chunks"])
    plan.close()
    rng = np.random.default_rng(9300 + m)
    for complex_ in (False, True):
        x, k = _signal32(rng, n), _kernel32(rng, m, complex_)
        x64, k64 = x.astype(np.float64), k.astype(np.complex128 if complex_ else np.float64)
        full = fftconvolve(x64, k64, mode="full")
        Y = sfft.fft(k64, f)
        for mode in sc.MODES:
            ref = _crop(full, n, m, mode)
            what = "refused grid m=%d %s %s" % (m, "complex" if complex_ else "real", mode)
            got = fastconv_hip(x, k, mode=mode, fft_length=f)
            assert got.dtype == (np.complex64 if complex_ else np.float32)
            _gate32(got, ref, CONV_TOL, what)
            got = fastconv_freq_hip(x, Y, m, mode=mode)
            assert got.dtype == (np.complex64 if complex_ else np.float32)
            _gate32(got, ref, CONV_TOL, what + " freq")
            assert np.allclose(fastconv_hip(x64, k64, mode=mode, fft_length=f, precision="high"), ref)
            assert np.allclose(fastconv_freq_hip(x64, Y, m, mode=mode, precision="high"), ref)


# ---- G. limits -------------------------------------------------------------------------------------------------------------
def test_admitted_limits():
    from ghost_amd._lib import GhostCwtError, ERR_INVALID, ERR_UNSUPPORTED
    from ghost_amd.sigtools import ConvPlan, analytic_signal_hip, chirpz_dft_hip, fastconv_hip, fastconv_freq_hip
    # 2 n - 1 <= 2^22 (n = 2^21 itself passes: test_dft_every_p1[1024])
    with pytest.raises(GhostCwtError, match="DFT length exceeds 2\\^21") as exc:
        chirpz_dft_hip(np.zeros(sc.G_DFT_MAX + 1, dtype=np.float32))
    assert exc.value.code == ERR_UNSUPPORTED
    with pytest.raises(GhostCwtError, match="fft_length exceeds 2\\^21") as exc:
        analytic_signal_hip(np.zeros(8, dtype=np.float32), fft_length=sc.G_DFT_MAX + 1)
    assert exc.value.code == ERR_UNSUPPORTED
    with pytest.raises(GhostCwtError, match="float64 DFT lengths up to 2\\^23") as exc:
        chirpz_dft_hip(np.zeros(sc.G_F64_MAX + 1), precision="high")
    assert exc.value.code == ERR_UNSUPPORTED
    # fft_length: 1 .. 2^22 in Python, fft_log2 0 or 12 .. 22 in C
    with pytest.raises(ValueError, match="fft_length must be between 1 and 2\\*\\*22"):
        ConvPlan(1000, 10, fft_length=2 ** 22 + 1)
    with pytest.raises(ValueError, match="fft_length must be between 1 and 2\\*\\*22"):
        ConvPlan(1000, 10, fft_length=0)
    small = ConvPlan(1000, 10, fft_length=1)
    assert (small.fft_length, small.chunk, small.n_chunks) == (4096, 4087, 1)
    small.close()
    top = ConvPlan(1000, 10, fft_length=2 ** 22)
    assert top.fft_length == 1 << 22
    top.close()
    for log2 in (1, 11, 23):
        rc, msg = _plan_create_rc(1000, 10, 1, log2)
        assert rc == ERR_INVALID and "fft_log2 must be 0 or 12..22" in msg, log2
    for log2 in (12, 22):
        assert _plan_create_rc(1000, 10, 1, log2)[0] == 0
    with pytest.raises(ValueError, match="FFT length must be at least the kernel size"):
        fastconv_hip(np.zeros(100), np.ones(20), fft_length=19)
    # empty and 2-D inputs: refused where the reference refuses
    x, k = np.ones(100), np.ones(10)
    for kw in ({}, {"precision": "high"}):
        with pytest.raises(ValueError, match="Signal must be 1D"):
            fastconv_hip(x.reshape(2, 50), k, **kw)
        with pytest.raises(ValueError, match="Kernel must be 1D"):
            fastconv_hip(x, k.reshape(2, 5), **kw)
        with pytest.raises(ValueError, match="Signal must be 1D"):
            fastconv_freq_hip(x.reshape(2, 50), np.fft.fft(k, 64), 10, **kw)
        with pytest.raises(ValueError, match="Kernel must be 1D"):
            fastconv_freq_hip(x, np.fft.fft(k, 64).reshape(2, 32), 10, **kw)
        with pytest.raises((ValueError, GhostCwtError)):
            fastconv_hip(np.zeros(0), k, **kw)
        with pytest.raises((ValueError, GhostCwtError)):
            fastconv_hip(x, np.zeros(0), **kw)
        with pytest.raises(ValueError, match="Data must be 1-dimensional"):
            chirpz_dft_hip(x.reshape(2, 50), **kw)
        with pytest.raises(ValueError, match="Data must not be empty"):
            chirpz_dft_hip(np.zeros(0), **kw)
        with pytest.raises(ValueError, match="Cannot compute analytic signal on an empty array"):
            analytic_signal_hip(np.zeros(0), **kw)
        with pytest.raises(ValueError, match="Input data must be 1-dimensional"):
            analytic_signal_hip(x.reshape(2, 50), **kw)
