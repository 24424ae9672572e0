"""Float64 NumPy twin of gcwt_coupling's definition (include/ghostcwt.h): binned phase-amplitude coupling inside a channel.

W (C, S, n_cols) complex; bin m holds the columns [m w, min((m + 1) w, n_cols)), B = ceil(n_cols / w) bins of cnt_m
columns.  For a channel c, a phase row p and an amplitude row a:
    u_p(t) = W[c,p,t] / |W[c,p,t]| (0 where that is 0),   M = sum_t |W[c,a,t]| u_p(t),   S = sum_t |W[c,a,t]|,
    vector = M / cnt,   mvl = |M| / S (0 where S == 0),   amplitude = S / cnt.

The bounds below are derived from the order csrc/coupling.hip prescribes, not measured.  u = 2^-24, L = ceil(w / 64).
"""
import numpy as np

U = 2.0 ** -24

# Roundings a term |w_a| u_p carries when it enters a lane's chain, each relative to the term (every operation is a
# single correctly rounded float32 one):
#   r2 = fmaf(im, im, re * re)    2   -> sqrt halves them: 1
#   |w| = sqrt(r2)                1   -> |w_p| carries 2, |w_a| carries 2
#   inv = 1 / |w_p|               1
#   u = (re * inv, im * inv)      1   -> a component of u carries 2 + 1 + 1 = 4
# The product |w_a| * u.x is made inside fmaf(|w_a|, u.x, acc) and rounds with the chain.  K = 4 + 2.
K = 6


def chain(window):
    """L: the columns a lane adds one after the other."""
    return -(-int(window) // 64)


def vector_bound(window):
    """|M_dev - M_ref| / S: per component K roundings in the terms, L in the lane's chain of fmaf, 6 in the tree and 1
    in the divide by cnt, each relative to at most sum |w_a| |u.x| <= S; sqrt(2) for the two components."""
    return np.sqrt(2.0) * (K + chain(window) + 6 + 1) * U


def amplitude_bound(window):
    """Relative: |w|'s 2 roundings, the chain of L additions, the tree of 6, the divide by cnt."""
    return (2 + chain(window) + 6 + 1) * U


def mvl_bound(window):
    """|M| / S with |M| / S <= 1: the vector's error, the amplitude's, and 3 for the modulus, its root and the divide."""
    return vector_bound(window) + amplitude_bound(window) + 3 * U


def bin_counts(n_cols, window):
    n_bins = -(-n_cols // window)
    return np.minimum(window, n_cols - np.arange(n_bins) * window)


def bin_sums(v, window):
    """Sums of v (..., n_cols) over the bins: (..., B), in v's (float64 / complex128) precision."""
    return np.add.reduceat(v, np.arange(0, v.shape[-1], window), axis=-1)


def unit(w):
    """w / |w|, 0 where |w| == 0."""
    w = np.asarray(w, dtype=np.complex128)
    r = np.abs(w)
    return np.where(r > 0, w / np.where(r > 0, r, 1.0), 0.0)


def model(w, phase_rows, amp_rows, window):
    """phase_rows, amp_rows: (first, count).  {"vector" (C, P, A, B) complex128, "mvl" (C, P, A, B), "amplitude"
    (C, A, B), "m" (C, P, A, B) and "s" (C, A, B): the raw sums, "ratio" (C, P, A, B): M / S, 0 where S == 0,
    "counts" (B,)}."""
    w = np.asarray(w, dtype=np.complex128)
    (p0, n_p), (a0, n_a) = phase_rows, amp_rows
    cnt = bin_counts(w.shape[-1], window)
    amp = np.abs(w[:, a0:a0 + n_a])                                              # C, A, n
    s = bin_sums(amp, window)
    m = np.stack([bin_sums(amp * unit(w[:, p:p + 1]), window) for p in range(p0, p0 + n_p)], axis=1)   # C, P, A, B
    s4 = np.broadcast_to(s[:, None], m.shape)
    ok = s4 > 0
    ratio = np.zeros_like(m)
    ratio[ok] = m[ok] / s4[ok]
    return {"vector": m / cnt, "mvl": np.abs(ratio), "amplitude": s / cnt, "m": m, "s": s, "ratio": ratio, "counts": cnt}


def coupled_input(n=32768, fs=1000.0):
    """Two channels of an 8 Hz rhythm with an 80 Hz one in noise (rng 7, drawn in channel order).  Channel 0: the 80 Hz
    amplitude is largest 1.0 rad after the 8 Hz peak (modulation depth 0.8); channel 1: constant 80 Hz amplitude."""
    rng = np.random.default_rng(7)
    t = np.arange(n) / fs
    th = 2 * np.pi * 8 * t
    x = np.empty((2, n))
    x[0] = np.sin(th + np.pi / 2) + 0.4 * 0.5 * (1 + 0.8 * np.cos(th - 1.0)) * np.sin(2 * np.pi * 80 * t) \
        + 0.2 * rng.standard_normal(n)
    x[1] = np.sin(th + np.pi / 2) + 0.2 * np.sin(2 * np.pi * 80 * t) + 0.2 * rng.standard_normal(n)
    return x


def gate_bound(w_ref, phase_rows, amp_rows, window):
    """How far M / S may move when every row of the float64 coefficients w_ref (C, S, n) moves by the project's gate,
    eps_r = 1e-5 max_t |W[r]| per sample: a phase unit vector turns by at most min(2, 2 eps_p / |W_p|), an amplitude
    moves by at most eps_a, and S in the denominator by cnt eps_a.  (C, P, A, B)."""
    w_ref = np.asarray(w_ref, dtype=np.complex128)
    (p0, n_p), (a0, n_a) = phase_rows, amp_rows
    eps = 1e-5 * np.abs(w_ref).max(axis=-1, keepdims=True)                       # C, S, 1
    ref = model(w_ref, phase_rows, amp_rows, window)
    amp = np.abs(w_ref[:, a0:a0 + n_a])
    turn = np.minimum(2.0, 2 * eps[:, p0:p0 + n_p] / np.maximum(np.abs(w_ref[:, p0:p0 + n_p]), 1e-300))   # C, P, n
    term = np.stack([bin_sums(amp * turn[:, i:i + 1], window) for i in range(n_p)], axis=1)              # C, P, A, B
    d_amp = (ref["counts"] * eps[:, a0:a0 + n_a])[:, None]                       # C, 1, A, B
    s = ref["s"][:, None]
    return (term + d_amp) / s + ref["mvl"] * d_amp / s
