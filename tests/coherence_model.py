"""Float64 NumPy twin of gcwt_coherence's definition (include/ghostcwt.h): binned cross-spectra of channel pairs.

W (C, S, n_cols) complex; bin m holds the columns [m w, min((m + 1) w, n_cols)), B = ceil(n_cols / w) bins of cnt_m
columns.  For a pair (a, b):  Sxy = sum W[a] conj(W[b]),  Sxx = sum |W[a]|^2,  Syy = sum |W[b]|^2 over the bin and
    cross = Sxy / cnt,   power = Sxx / cnt (every channel),   coherence = |Sxy|^2 / (Sxx Syy), 0 where Sxx Syy == 0.
"""
import numpy as np


def all_pairs(n_channels):
    return np.array([(a, b) for a in range(n_channels) for b in range(a + 1, n_channels)], dtype=np.int64).reshape(-1, 2)


def seed_pairs(seed, n_channels):
    return np.array([(seed, k) for k in range(n_channels) if k != seed], dtype=np.int64).reshape(-1, 2)


def bin_counts(n_cols, window):
    n_bins = -(-n_cols // window)
    return np.minimum(window, n_cols - np.arange(n_bins) * window)


def bin_sums(v, window):
    """Sums of v (..., n_cols) over the bins: (..., B), in v's (float64 / complex128) precision."""
    n_cols = v.shape[-1]
    return np.add.reduceat(v, np.arange(0, n_cols, window), axis=-1)


def model(w, pairs, window):
    """{"cross" (P, S, B) complex128, "power" (C, S, B), "coherence" (P, S, B), "sxy", "sxx" (C, S, B): the raw sums,
    "gamma" (P, S, B): Sxy / sqrt(Sxx Syy), 0 where Sxx Syy == 0, "counts" (B,)}."""
    w = np.asarray(w, dtype=np.complex128)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    cnt = bin_counts(w.shape[-1], window)
    sxx = bin_sums(w.real ** 2 + w.imag ** 2, window)
    sxy = np.stack([bin_sums(w[a] * np.conj(w[b]), window) for a, b in pairs]) if len(pairs) else \
        np.zeros((0,) + sxx.shape[1:], np.complex128)
    den = sxx[pairs[:, 0]] * sxx[pairs[:, 1]]
    ok = den > 0
    gamma = np.zeros_like(sxy)
    gamma[ok] = sxy[ok] / np.sqrt(den[ok])
    return {"cross": sxy / cnt, "power": sxx / cnt, "coherence": np.abs(gamma) ** 2, "gamma": gamma, "sxy": sxy,
            "sxx": sxx, "counts": cnt}


def gamma_of(cross, power, pairs):
    """gamma = cross / sqrt(power_a power_b) in float64 from (device) outputs; 0 where the product is 0."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    cross = np.asarray(cross, dtype=np.complex128)
    power = np.asarray(power, dtype=np.float64)
    den = power[pairs[:, 0]] * power[pairs[:, 1]]
    ok = den > 0
    g = np.zeros_like(cross)
    g[ok] = cross[ok] / np.sqrt(den[ok])
    return g


def gamma_bound(window):
    """Worst-case float32 rounding of the prescribed order, relative to sqrt(Sxx Syy): a lane's chain of
    2 ceil(w / 64) fused multiply-adds per component, a tree of 6, the final divide and root, times sqrt(2) + 1 for the
    complex modulus and the two normalisers (rounded up to 3)."""
    return 3 * (2 * -(-window // 64) + 8) * 2.0 ** -24


def power_bound(window):
    """Relative: a chain of ceil(w / 64) additions of |w|^2, the tree, the divide."""
    return (-(-window // 64) + 8) * 2.0 ** -24


def three_channel_input(n=32768, fs=1000.0):
    """Two 8 Hz sines 0.7 rad apart in noise and a channel of noise alone (rng 7, drawn in channel order)."""
    rng = np.random.default_rng(7)
    t = np.arange(n) / fs
    x = np.empty((3, n))
    x[0] = np.sin(2 * np.pi * 8 * t) + 0.5 * rng.standard_normal(n)
    x[1] = np.sin(2 * np.pi * 8 * t - 0.7) + 0.5 * rng.standard_normal(n)
    x[2] = 0.5 * rng.standard_normal(n)
    return x
