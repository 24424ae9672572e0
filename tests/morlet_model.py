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
