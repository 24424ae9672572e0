"""Float64 NumPy twin of gcwt_bandpass's definition (include/ghostcwt.h): band-limited analytic signals.

W (C, S, n_cols) complex; a band is the rows first .. first + R - 1; g, h: (S,) weights.  For a channel c, a band and a
column t:
    analytic = sum_r g_r W[c, r, t],   envelope = |analytic|,   power = sum_r h_r |W[c, r, t]|^2.

The bounds below are derived from the order csrc/bandpass.hip prescribes, not measured.  u = 2^-24, R rows in the band,
every operation a single correctly rounded float32 one, each sum a chain from an exact 0 along the band's rows:
    re = fmaf(g_r, w_r.re, re)                 R roundings, each relative to a partial sum that is at most
                                               sum_r |g_r| |w_r.re| in modulus (to first order in u)
    p  = fmaf(h_r, norm2(w_r), p)              norm2 = fmaf(im, im, re * re) carries 2; the chain R; all terms >= 0
    envelope = sqrt(fmaf(im, im, re * re))     norm2 carries 2, the root halves them and adds its own: 1 + 1 = 2
"""
import numpy as np

U = 2.0 ** -24


def analytic_bound(count):
    """|z_dev - z| / T with T = sum_r |g_r| |w_r|: per component the chain of R fmaf, each rounding relative to a partial
    sum of modulus at most sum_r |g_r| |w_r.x| <= T; sqrt(2) for the two components."""
    return np.sqrt(2.0) * int(count) * U


def envelope_extra():
    """What the modulus adds to the analytic bound, relative to |z|: norm2's two roundings, halved by the root, and the
    root's own."""
    return 2 * U


def power_bound(count):
    """Relative: norm2's 2 roundings in every term and the chain of R fmaf over terms that are all >= 0 (h >= 0), so
    every partial sum is at most the whole."""
    return (2 + int(count)) * U


def band_terms(w, bands, g):
    """T = sum_r |g_r| |w_r|, (C, B, n): what analytic_bound is relative to."""
    w = np.asarray(w, dtype=np.complex128)
    g = np.abs(np.asarray(g, dtype=np.float64))
    return np.stack([np.tensordot(g[a:a + n], np.abs(w[:, a:a + n]), axes=(0, 1)) for a, n in bands], axis=1)


def model(w, bands, g, h):
    """bands: (B, 2) of (first, count).  {"analytic" (C, B, n) complex128, "envelope", "power" (C, B, n) float64}, g and h
    taken as the float64 values of what they hold."""
    w = np.asarray(w, dtype=np.complex128)
    g, h = np.asarray(g, dtype=np.float64), np.asarray(h, dtype=np.float64)
    z = np.stack([np.tensordot(g[a:a + n], w[:, a:a + n], axes=(0, 1)) for a, n in bands], axis=1)
    p = np.stack([np.tensordot(h[a:a + n], np.abs(w[:, a:a + n]) ** 2, axes=(0, 1)) for a, n in bands], axis=1)
    return {"analytic": z, "envelope": np.abs(z), "power": p}


def fmaf32(a, b, c):
    """float32(a * b + c) with a single rounding, for float32 arrays: the product of two float32 is exact in float64; its
    sum with c is made in float64 and, where that was inexact, rounded to odd (two_sum gives the error), which the cast to
    float32 -- 29 bits fewer -- then rounds as it would the exact sum."""
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    bits = s.view(np.int64) if s.ndim else np.array(s).view(np.int64)
    fix = (err != 0) & (bits & 1 == 0) & np.isfinite(s)
    toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where(fix, np.nextafter(s, toward), s)
    return s.astype(np.float32)


def norm2_32(z):
    """wave_reduce.h's norm2 of complex64 values, bit for bit: fmaf(im, im, re * re)."""
    z = np.asarray(z, dtype=np.complex64)
    return fmaf32(z.imag, z.imag, z.real * z.real)                  # (float32 * float32 in NumPy: one rounding)


def chains32(w, bands, g, h):
    """The prescribed float32 chains themselves, bit for bit, for complex64 w: {"analytic" complex64, "envelope",
    "power" float32}, each (C, B, n)."""
    w = np.asarray(w, dtype=np.complex64)
    g, h = np.asarray(g, dtype=np.float32), np.asarray(h, dtype=np.float32)
    c, _, n = w.shape
    out = {"analytic": np.zeros((c, len(bands), n), np.complex64), "envelope": np.zeros((c, len(bands), n), np.float32),
           "power": np.zeros((c, len(bands), n), np.float32)}
    for k, (a, cnt) in enumerate(bands):
        re = im = p = np.zeros((c, n), np.float32)
        for r in range(a, a + cnt):
            re = fmaf32(g[r], w[:, r].real, re)
            im = fmaf32(g[r], w[:, r].imag, im)
            p = fmaf32(h[r], norm2_32(w[:, r]), p)
        out["analytic"][:, k] = re + 1j * im
        out["envelope"][:, k] = np.sqrt(norm2_32(out["analytic"][:, k]))
        out["power"][:, k] = p
    return out


def gate_bound(w_ref, bands, g, h):
    """How far analytic and power may move when every row of the float64 coefficients w_ref (C, S, n) moves by the
    project's gate, eps_r = 1e-5 max_t |W[r]| per sample: analytic by sum_r |g_r| eps_r, power by sum_r h_r (2 |W_r| eps_r
    + eps_r^2).  -> (analytic (C, B, 1), power (C, B, n))."""
    w_ref = np.asarray(w_ref, dtype=np.complex128)
    g, h = np.abs(np.asarray(g, dtype=np.float64)), np.asarray(h, dtype=np.float64)
    eps = 1e-5 * np.abs(w_ref).max(axis=-1, keepdims=True)                       # C, S, 1
    za = np.stack([np.tensordot(g[a:a + n], eps[:, a:a + n], axes=(0, 1)) for a, n in bands], axis=1)
    pw = np.stack([np.tensordot(h[a:a + n], 2 * np.abs(w_ref[:, a:a + n]) * eps[:, a:a + n] + eps[:, a:a + n] ** 2, axes=(0, 1))
                   for a, n in bands], axis=1)
    return za, pw


def tone(n=16384, fs=1000.0, f0=20.0, amplitude=0.7):
    """The sinusoid the normalisation is checked on."""
    return amplitude * np.cos(2 * np.pi * f0 * np.arange(n) / fs + 0.3)
