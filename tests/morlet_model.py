"""Float64 model of the Morlet kernel's frequency response, written from the formula ("Morlet"), not
from the library's code.

For Morlet(w0, freq, fs).get_wavelet() (ghost_amd/wave/morlet.py): sigma = scale fs, M = 15 sigma, L = ceil(M + 1)
taps, the wavelet's centre at array index c0 = (M + 1) / 2, delay d = c0 - (L - 1) // 2 against the origin of 'same'
mode.  With F(xi) = sqrt(2 pi) (exp(-(xi - w0)^2 / 2) - exp(-w0^2 / 2) exp(-xi^2 / 2)),

    H(theta) = sum_n psi[n] exp(-i theta (n - (L - 1) // 2))
             = exp(-i theta d) pi^(-1/4) sqrt(sigma) sum_k exp(-2 pi i k c0) F(sigma (theta + 2 pi k)).
"""
import numpy as np


def geometry(w0, freq, fs):
    """(sigma, M, L, c0, d) of the kernel at ``freq`` Hz."""
    scale = (w0 + np.sqrt(2 + w0 ** 2)) / (4 * np.pi * freq)
    sigma = scale * fs
    m = 15 * fs * scale
    length = int(np.ceil(m + 1))
    c0 = (m + 1) / 2
    return sigma, m, length, c0, c0 - (length - 1) // 2


def shape(xi, w0):
    """F(xi): the transform of the continuous wavelet at unit scale."""
    return np.sqrt(2 * np.pi) * (np.exp(-0.5 * (xi - w0) ** 2) - np.exp(-0.5 * w0 ** 2) * np.exp(-0.5 * xi ** 2))


def response(theta, w0, freq, fs, aliases=3):
    """H(theta) of the L-tap kernel, ``aliases`` terms either side of k = 0."""
    sigma, _, _, c0, d = geometry(w0, freq, fs)
    theta = np.asarray(theta, dtype=np.float64)
    acc = np.zeros(theta.shape, dtype=np.complex128)
    for k in range(-aliases, aliases + 1):
        acc += np.exp(-2j * np.pi * k * c0) * shape(sigma * (theta + 2 * np.pi * k), w0)
    return np.exp(-1j * theta * d) * np.pi ** -0.25 * np.sqrt(sigma) * acc


def dtft(psi, theta):
    """sum_n psi[n] exp(-i theta (n - (L - 1) // 2)) by direct summation."""
    n = np.arange(len(psi)) - (len(psi) - 1) // 2
    return np.exp(-1j * np.outer(np.asarray(theta, dtype=np.float64), n)) @ np.asarray(psi)


def band(w0, tol):
    """(xi_hi, xi_neg): outside [-xi_neg, xi_hi] the un-aliased |F| stays below ``tol`` of its peak (xi = sigma theta,
    the same for every scale); xi_neg = 0 when nothing below zero frequency reaches ``tol``.  By dense sampling."""
    xi = np.linspace(-20.0, w0 + 20.0, 4000001)
    f = np.abs(shape(xi, w0))
    above = np.nonzero(f > tol * f.max())[0]
    step = xi[1] - xi[0]
    xi_hi = xi[above[-1]] + step
    xi_neg = max(0.0, -(xi[above[0]] - step))
    return xi_hi, xi_neg


def cwt_decimated(x, fs, freqs_hz, w0, epoch_bounds=None, plan=None, rows=None, B=256):
    """Float64 model of what the engine computes for a Morlet plan, complex128 (len(rows), N): the structure of
    decimated_model.cwt_decimated with H_s the closed form above.  The decisions -- method,
    decimation, halo, hop per scale; band shift and low cut per level, a level found by (decimation, halo, hop) since
    a Morlet plan can hold two levels of one decimation; FFT length per epoch -- are the planner's own (``plan``:
    a CwtPlan of the layout, made here when omitted).  Whole epochs only (no time blocks)."""
    import math
    from scipy.fft import fft, ifft
    from decimated_model import low_cut
    from ghost_amd.engine import CwtPlan
    from ghost_amd.wave import Morlet
    from oracle import ghost_oracle as orc
    x = np.asarray(x).squeeze().astype(np.float64)
    x = x - x.mean()
    n = x.size
    epoch_bounds = np.array([[0, n]]) if epoch_bounds is None else np.asarray(epoch_bounds).reshape(-1, 2)
    freqs_hz = np.atleast_1d(np.asarray(freqs_hz, dtype=np.float64))
    if plan is None:
        plan = CwtPlan(n, 1, fs, freqs_hz, morlet_w0=w0, epoch_bounds=epoch_bounds, output="complex")
    rows = list(range(len(freqs_hz))) if rows is None else list(rows)
    si = plan.scale_info()
    level_of = {(lv["decimation"], lv["halo"], lv["hop"]): lv for lv in plan.debug_levels()}
    fft_len = {(a, b): p for (a, b, p) in plan.segments()}
    out = np.zeros((len(rows), n), dtype=np.complex128)
    k = np.arange(B)
    for start, stop in epoch_bounds:
        ne = stop - start
        p_big = fft_len[(start, stop)]
        lead = start - (start & ~63)                   # segments start on multiples of 64 samples
        X = fft(np.concatenate([np.zeros(lead), x[start:stop]]), n=p_big)
        xr_cache = {}
        for o, i in enumerate(rows):
            f, method = freqs_hz[i], si["method"][i]
            if method in (1, 3):                       # time domain / block convolution: the literal kernel
                psi = Morlet(w0=w0, freq=f, fs=fs).get_wavelet()
                assert len(psi) == si["length"][i]
                out[o, start:stop] = orc.overlap_add_convolve(x[start:stop], psi)
                continue
            if method == 2:                            # full band
                H = response(2 * np.pi * np.arange(p_big) / p_big, w0, f, fs)
                out[o, start:stop] = ifft(X * H)[lead:lead + ne]
                continue
            key = (int(si["decimation"][i]), int(si["halo"][i]), int(si["hop"][i]))
            R, lh, hop = key
            lv = level_of[key]
            shift, M = lv["band_shift"], p_big // R
            if key not in xr_cache:
                sl = X[(np.arange(M) - shift * M // B) % p_big]
                if not shift:
                    sl = sl * low_cut(lv["low_cut"], p_big, M)
                xr_cache[key] = ifft(sl) / R           # x_R: bin u stands for frequency u - shift M / B
            xr = xr_cache[key]
            H = response(2 * np.pi * (k - shift) / (B * R), w0, f, fs)
            tw = np.exp(2j * np.pi * np.outer(k - shift, np.arange(R)) / (B * R))
            nblk = int(math.ceil(math.ceil((lead + ne) / R) / hop))
            first = np.arange(nblk) * hop - lh
            XB = fft(xr[(first[:, None] + k[None, :]) % M], axis=1)
            blk = ifft((XB * H)[:, :, None] * tw[None], axis=1)                    # [b, m, r]
            if shift:      # the carrier of the shifted band: block position and sample within the block
                blk = blk * np.exp(-2j * np.pi * shift * (first[:, None] + k[None, :]) / B)[:, :, None]
            y = blk[:, lh:lh + hop, :].reshape(-1)
            out[o, start:stop] = y[lead:lead + ne]
    return out
