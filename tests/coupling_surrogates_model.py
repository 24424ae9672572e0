"""Float64 NumPy twin of gcwt_coupling_surrogates' definition (include/ghostcwt.h): shift surrogates of coupling()'s mvl.

Bins, u_p, |w_a|, M, S and cnt are those of coupling_model.  For a shift L the surrogate of a bin with first column b and
cnt columns moves the amplitude row circularly inside the bin:
    M_L = sum_{r=0}^{cnt-1} |W[c,a, b + (r + L') mod cnt]| u_p(b + r),   L' = L mod cnt,   mvl_L = |M_L| / S (0 where S == 0);
over the K shifts of the list  mean = T / K,  sd = sqrt(max(0, (Q - T^2 / K) / (K - 1))),  T = sum mvl_k,  Q = sum mvl_k^2,
and count = the number of k with mvl_k >= mvl at L = 0.

The bounds below are derived from the order csrc/coupling_surrogates.hip prescribes, not measured.
"""
import numpy as np

import coupling_model as pm

U = 2.0 ** -24                                             # float32
E = 2.0 ** -53                                             # float64


def surrogate_bound(window):
    """|mvl_L dev - ref|: a surrogate is made by the operations of coupling()'s mvl in the same order -- the terms, a
    lane's chain of ceil(w / 64) fused multiply-adds, the tree, the modulus and the divide -- on other pairs of numbers."""
    return pm.mvl_bound(window)


def mean_rounding(k):
    """The device's mean against the float64 mean of the float32 surrogates it returned, all in [0, 1]: T is a float64
    sum of K exact terms in some fixed order (relative K 2^-53, and T / K <= 1), the divide by K is inside that, and the
    result is rounded to float32 once (2^-24 of a value <= 1)."""
    return k * E + U


def mean_bound(window, k):
    """... against the model: the mean of the surrogates' own errors, each at most surrogate_bound, on top."""
    return surrogate_bound(window) + mean_rounding(k)


def sd_rounding(k):
    """The device's sd against the float64 sd (K - 1) of the float32 surrogates v_k it returned, all in [0, 1].  With e =
    2^-53: Q^ = Q (1 + t), |t| <= K e (the squares of float32 numbers are exact in float64, K additions); T^ = T (1 + t'),
    |t'| <= K e; T^2 / K takes two more roundings, so it is off by at most (2 K + 2) e T^2 / K; the subtraction D = Q - T^2 /
    K adds e D.  Q, T^2 / K and D are all at most K, so |D^ - D| <= e K (K + 2 K + 2 + 1) = e K (3 K + 3).  The divide by
    K - 1 adds e var: |var^ - var| <= e (K (3 K + 3) / (K - 1) + 1).  The clamp at 0 only helps (var >= 0).  The root:
    |sqrt(a) - sqrt(b)| <= sqrt(|a - b|), its own rounding e, and the rounding to float32, 2^-24 of a value below 1 (the sd
    of K numbers in [0, 1] is at most sqrt(K / (K - 1)) / 2)."""
    return np.sqrt(E * (k * (3.0 * k + 3.0) / (k - 1.0) + 1.0)) + E + U


def sd_bound(window, k):
    """... against the model: the sample sd is a seminorm, so moving every surrogate by at most b = surrogate_bound moves
    it by at most the sd of the moves, sqrt(sum d_k^2 / (K - 1)) <= b sqrt(K / (K - 1))."""
    return np.sqrt(k / (k - 1.0)) * surrogate_bound(window) + sd_rounding(k)


def shifted_sums(w, phase_rows, amp_rows, window, shifts):
    """M_L of every shift: (K, C, P, A, B) complex128, and S: (C, A, B)."""
    w = np.asarray(w, dtype=np.complex128)
    (p0, n_p), (a0, n_a) = phase_rows, amp_rows
    n = w.shape[-1]
    n_full, n_bins = n // window, -(-n // window)
    u = pm.unit(w[:, p0:p0 + n_p])                                               # C, P, n
    amp = np.abs(w[:, a0:a0 + n_a])                                              # C, A, n
    m = np.zeros((len(shifts), w.shape[0], n_p, n_a, n_bins), dtype=np.complex128)
    pieces = []
    if n_full:
        pieces.append((slice(0, n_full), window, u[..., :n_full * window].reshape(w.shape[0], n_p, n_full, window),
                       amp[..., :n_full * window].reshape(w.shape[0], n_a, n_full, window)))
    if n_bins > n_full:
        cnt = n - n_full * window
        pieces.append((slice(n_full, n_bins), cnt, u[..., n_full * window:].reshape(w.shape[0], n_p, 1, cnt),
                       amp[..., n_full * window:].reshape(w.shape[0], n_a, 1, cnt)))
    for where, cnt, ub, ab in pieces:
        for k, shift in enumerate(shifts):
            idx = (np.arange(cnt) + int(shift) % cnt) % cnt
            m[k, :, :, :, where] = np.einsum("cpbr,cabr->cpab", ub, ab[..., idx])
    return m, pm.bin_sums(amp, window)


def model(w, phase_rows, amp_rows, window, shifts):
    """phase_rows, amp_rows: (first, count); shifts: K integers in [0, window).  {"mvl" (K, C, P, A, B): every surrogate,
    "mean" and "sd" (C, P, A, B), "count" (C, P, A, B) int: the surrogates >= the L = 0 value, "observed" (C, P, A, B): that
    value, "s" (C, A, B)}."""
    m, s = shifted_sums(w, phase_rows, amp_rows, window, list(shifts) + [0])   # (the L = 0 value by the same sums)
    s5 = np.broadcast_to(s[None, :, None], m.shape)
    mvl = np.zeros(m.shape)
    ok = s5 > 0
    mvl[ok] = np.abs(m[ok]) / s5[ok]
    mvl, observed = mvl[:-1], mvl[-1]
    return {"mvl": mvl, "mean": mvl.mean(axis=0), "sd": mvl.std(axis=0, ddof=1), "count": (mvl >= observed[None]).sum(axis=0),
            "observed": observed, "s": s}


def z_and_p(observed, mean, sd, count, k):
    """z = (observed - mean) / sd in float64, 0 where sd == 0; p = (1 + count) / (K + 1)."""
    observed, mean, sd = (np.asarray(v, dtype=np.float64) for v in (observed, mean, sd))
    z = np.where(sd > 0, (observed - mean) / np.where(sd > 0, sd, 1.0), 0.0)
    return z, (1.0 + np.asarray(count)) / (k + 1.0)


def jittered_input(n=32768, fs=1000.0, seed=7):
    """Two channels of a rhythm near 8 Hz whose frequency wanders (an AR(1) deviation of sd 1.5 Hz and 0.25 s memory, so a
    bin of 2 s spans several coherence times of the phase) with an 80 Hz one in noise.  Channel 0: the 80 Hz amplitude is
    largest 1.0 rad after the slow peak (modulation depth 0.8); channel 1: constant 80 Hz amplitude.  The noise is drawn
    in channel order after the deviation."""
    rng = np.random.default_rng(seed)
    a = np.exp(-1.0 / 250.0)
    e = rng.standard_normal(n) * 1.5 * np.sqrt(1.0 - a * a)
    d = np.empty(n)
    d[0] = e[0]
    for i in range(1, n):
        d[i] = a * d[i - 1] + e[i]
    t = np.arange(n) / fs
    th = 2 * np.pi * np.cumsum(8.0 + d) / fs
    x = np.empty((2, n))
    x[0] = np.cos(th) + 0.2 * (1 + 0.8 * np.cos(th - 1.0)) * np.sin(2 * np.pi * 80 * t) + 0.2 * rng.standard_normal(n)
    x[1] = np.cos(th) + 0.2 * np.sin(2 * np.pi * 80 * t) + 0.2 * rng.standard_normal(n)
    return x
