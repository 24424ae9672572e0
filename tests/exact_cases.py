"""Shared pieces of the tests of the three paths that compute a scale without a decimated band (plain module, no
fixtures, no GPU): the full band (GCWT_SCALE_FULLBAND: k_fullband_filter, k_fullband_rows, k_fullband4,
k_fullband_cols256 / colsq, launch_fft_cols + k_fullband_store), the block convolution (GCWT_SCALE_BLOCKCONV:
k_bc_forward, k_bc_scales) and the time domain (GCWT_SCALE_DIRECT: k_build_direct, k_direct).  The cases, seeded
recordings, float64 models of each path and the single-precision references the tighter gates are taken from
(tests/test_exact_cases_cpu.py pins the planner's decisions and shows what the comparison catches,
tests/test_gpu_exact_matrix.py runs the cases; profiles/exact_matrix.md has the measurements).

All cases: 1 kHz, float32 recordings.  Full band: option blockconv = 0, Morse(3, 2) (F4x: Morse(3, 20)).

Case  plan                                                          what it is there for
F1    n = 3000, C = 3, [30, 12, 9], two epochs                      P1 = 1 twice in one batch (6 slots), leads 7 and
                                                                    3, no column pass; the 30 Hz scale is time domain
F2    n = 6000, C = 2, f2                                           P1 = 2
F4    n = 12001, C = 2, f9                                          P1 = 4, sets 4 + 4 + 1, k_fullband4 and, with
                                                                    option fullband4 = 0, the two-pass kernels
F8    n = 30000, C = 2, f2, precision default, fast, exact          P1 = 8; exact: 491 taps by blocks with a ramp
F64   n = 400000, C = 2, f9, two epochs                             P1 = 64, one batch of two segments, group 32 < P1
F128  n = 400000, C = 3, f2                                         P1 = 128, 3 slots, per = 96
F256  n = 600000, C = 2, f2, three output modes                     k_fullband_cols256 and its tile order
F4x   Morse(3, 20), n = 200000, C = 36, [9, 6, 4, 2.5], exact,      22 segments of 2^14 points in batches (0, 16),
      max_fft_log2 = 14, amplitude                                  (16, 6): 576 slots, the set split 3 of 4, so one
                                                                    workgroup of k_fullband4 makes two scales

Block convolution: Morse(3, 3), option direct_max_len = 48.
B1    n = 60000, C = 3, nine scales of 19 .. 2456 taps, five epochs groups (hop 3456, back 320) x 4 and (hop 1536, back
                                                                    1280) x 3; an epoch starting mid-block, one shorter
                                                                    than a block, one on an odd block and shorter than
                                                                    back, two that touch on a block edge
B2    n = 40000, C = 1, [61, 9], 17 epochs of 9 .. 6000 samples     two flushes (kSegBatch = 16)
B3    B1 with option bc_chunk_blocks = 2 and 6                      every pair its own launch; chunk seams
B4    B1's first group alone, C = 1 and C = 5                       blockIdx.x % n_channels

Time domain: option direct_max_len = 256, n = 6200, C = 3, Morse(3, 20) lengths 33 .. 48 (every residue of
(L - 1) // 2 mod 8) and Morse(2, 2) up to 241 taps.
D1    epochs [0, 2501), [2503, n)                                   the layout of test_time_domain_kernel_every_...
D2    D1's second epoch cut to 9 samples                            an epoch far shorter than the kernel
D3    17 epochs                                                     two launches"""
import numpy as np
from scipy.fft import fft, ifft

import level_cases as lc
from decimated_model import exact_gain
from oracle import ghost_oracle as orc

FS = 1000.0
ROW = lc.ROW
TOL = 1e-5                      # the project's gate on conftest.rel_err (2 TOL on power rows)
SEG_BATCH = 16                  # kernels.h: kSegBatch
METHOD_DIRECT, METHOD_FULLBAND, METHOD_BLOCKCONV = 1, 2, 3       # include/ghostcwt.h: GCWT_SCALE_*
BC_RAMP = 256                   # planner.h: kBlockConvRamp (precision = exact)

F9 = [12.0, 9.5, 8.0, 7.0, 5.5, 4.4, 3.1, 2.6, 2.2]
F2 = [9.0, 2.5]
_B1_F = [300.0, 140.0, 61.0, 33.0, 17.0, 9.0, 4.1, 2.7, 2.2]
_B1_EPOCHS = [[70, 21000], [21013, 22500], [24192, 24232], [30000, 41472], [41472, 59990]]


def _b2_epochs():
    lens = [9, 6000, 17, 1500, 3456, 40, 2999, 64, 1537, 100, 3000, 9, 4000, 333, 1536, 2048, 1000]
    out, at = [], 5
    for i, ln in enumerate(lens):
        out.append([at, at + ln])
        at += ln + (0 if i == 7 else 3 + 11 * (i % 4))          # (epochs 7 and 8 touch)
    return out


def _short_grid():
    """Morse(3, 20): one frequency per kernel length 33 .. 48 (the highest of each length)."""
    grid = np.linspace(0.30 * FS, 0.46 * FS, 4001)
    lens = orc.morse_lengths(orc.hz_to_rad(grid, FS))
    return np.array([grid[lens == L].max() for L in range(33, 49) if np.any(lens == L)])[::-1]


_D_LONG = [330.0, 97.0, 60.0, 40.0, 26.0, 15.0]
_D3_EPOCHS = [[3 + 365 * i, 3 + 365 * i + (9 if i == 4 else 200 + 7 * i)] for i in range(17)]

_FB = dict(gamma=3.0, beta=2.0, options={"blockconv": 0}, precisions=("default",), outputs=("complex",), epochs=None,
           max_fft_log2=0)
_BC = dict(gamma=3.0, beta=3.0, options={"direct_max_len": 48}, precisions=("high",), outputs=("complex",), epochs=None,
           max_fft_log2=0)
_TD = dict(n=6200, channels=3, options={"direct_max_len": 256}, precisions=("default",),
           outputs=("complex", "amplitude", "power"), max_fft_log2=0)
CASES = {
    "F1": dict(_FB, n=3000, channels=3, f=[30.0, 12.0, 9.0], epochs=[[7, 1400], [1411, 2990]]),
    "F2": dict(_FB, n=6000, channels=2, f=F2, outputs=("complex", "amplitude", "power")),
    "F4": dict(_FB, n=12001, channels=2, f=F9, outputs=("complex", "amplitude", "power")),
    "F8": dict(_FB, n=30000, channels=2, f=F2, precisions=("default", "fast", "exact")),
    "F64": dict(_FB, n=400000, channels=2, f=F9, epochs=[[5, 199000], [199047, 399990]]),
    "F128": dict(_FB, n=400000, channels=3, f=F2),
    "F256": dict(_FB, n=600000, channels=2, f=F2, outputs=("complex", "amplitude", "power")),
    "F4x": dict(_FB, n=200000, channels=36, f=[9.0, 6.0, 4.0, 2.5], beta=20.0, precisions=("exact",),
                outputs=("amplitude",), max_fft_log2=14),
    "B1": dict(_BC, n=60000, channels=3, f=_B1_F, epochs=_B1_EPOCHS, precisions=("high", "fast", "exact"),
               outputs=("complex", "amplitude", "power")),
    "B2": dict(_BC, n=40000, channels=1, f=[61.0, 9.0], epochs=_b2_epochs()),
    "B4-1": dict(_BC, n=60000, channels=1, f=_B1_F[2:6], epochs=_B1_EPOCHS),
    "B4-5": dict(_BC, n=60000, channels=5, f=_B1_F[2:6], epochs=_B1_EPOCHS),
    "D1s": dict(_TD, f=_short_grid(), gamma=3.0, beta=20.0, epochs=[[0, 2501], [2503, 6200]]),
    "D1l": dict(_TD, f=_D_LONG, gamma=2.0, beta=2.0, epochs=[[0, 2501], [2503, 6200]]),
    "D2": dict(_TD, f=_D_LONG, gamma=2.0, beta=2.0, epochs=[[0, 2501], [2503, 2512]], outputs=("complex",)),
    "D3": dict(_TD, f=_D_LONG, gamma=2.0, beta=2.0, epochs=_D3_EPOCHS, outputs=("complex",)),
}
FULLBAND_CASES = ("F1", "F2", "F4", "F8", "F64", "F128", "F256")           # one-batch plans: own-input comparison
DIRECT_CASES = ("D1s", "D1l", "D2", "D3")
GROUP_CASES = {"F64": (1, 8, 64, 3), "F128": (1, 8, 128, 3)}                # option fullband_group; 3 divides neither
F4_SUBSETS = ([1], [1, 2], [0, 1, 2])                                        # sets of 1, 2 and 3 scales
B1_RANGES = [(20000, 11000), (24191, 3), (41471, 2), (3456, 3456)]          # execute_block (start, length)
CHUNKS = (2, 6)                                                               # option bc_chunk_blocks (B3)

# What the planner decides per case (first precision of the case): FFT length, P1, launch batches, method per scale,
# kernel lengths, groups of the block convolution as (hop, back, scales).  Checked on a CPU build; the CPU file pins it.
_F9_LEN = [368, 465, 552, 631, 802, 1003, 1423, 1697, 2005]
_B1_LEN = [19, 39, 89, 164, 318, 601, 1318, 2001, 2456]
EXPECT = {
    "F1": dict(p=1 << 12, p1=1, batches=[(0, 2)], methods=[1, 2, 2], lengths=[148, 368, 491], groups=[]),
    "F2": dict(p=1 << 13, p1=2, batches=[(0, 1)], methods=[2, 2], lengths=[491, 1765], groups=[]),
    "F4": dict(p=1 << 14, p1=4, batches=[(0, 1)], methods=[2] * 9, lengths=_F9_LEN, groups=[]),
    "F8": dict(p=1 << 15, p1=8, batches=[(0, 1)], methods=[2, 2], lengths=[491, 1765], groups=[]),
    "F64": dict(p=1 << 18, p1=64, batches=[(0, 2)], methods=[2] * 9, lengths=_F9_LEN, groups=[]),
    "F128": dict(p=1 << 19, p1=128, batches=[(0, 1)], methods=[2, 2], lengths=[491, 1765], groups=[]),
    "F256": dict(p=1 << 20, p1=256, batches=[(0, 1)], methods=[2, 2], lengths=[491, 1765], groups=[]),
    "F4x": dict(p=1 << 14, p1=4, batches=[(0, 16), (16, 6)], methods=[2] * 4, lengths=[1550, 2325, 3487, 5580], groups=[]),
    "B1": dict(p=None, p1=None, batches=None, methods=[1, 1, 3, 3, 3, 3, 3, 3, 3], lengths=_B1_LEN,
               groups=[(3456, 320, [2, 3, 4, 5]), (1536, 1280, [6, 7, 8])]),
    "B2": dict(p=None, p1=None, batches=None, methods=[3, 3], lengths=[89, 601], groups=[(3456, 320, [0, 1])]),
    "B4-1": dict(p=None, p1=None, batches=None, methods=[3] * 4, lengths=_B1_LEN[2:6], groups=[(3456, 320, [0, 1, 2, 3])]),
    "B4-5": dict(p=None, p1=None, batches=None, methods=[3] * 4, lengths=_B1_LEN[2:6], groups=[(3456, 320, [0, 1, 2, 3])]),
}


class options:
    """Library switches for the plans made inside the ``with`` (they are read when a plan is created)."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        from ghost_amd.engine import set_option
        for k, v in self.kw.items():
            set_option(k, v)

    def __exit__(self, *exc):
        from ghost_amd.engine import set_option
        for k in self.kw:
            set_option(k, None)


def epochs_of(name):
    c = CASES[name]
    return np.array([[0, c["n"]]] if c["epochs"] is None else c["epochs"], dtype=np.int64)


def make_plan(name, precision=None, output="complex", n_channels=None, scales=None, **extra):
    """The case's plan; ``scales``: only these of its frequencies; ``extra``: further library options."""
    from ghost_amd.engine import CwtPlan
    c = CASES[name]
    precision = c["precisions"][0] if precision is None else precision
    f = np.asarray(c["f"], dtype=np.float64)
    with options(**dict(c["options"], **extra)):
        return CwtPlan(c["n"], c["channels"] if n_channels is None else n_channels, FS, f if scales is None else f[scales],
                       gamma=c["gamma"], beta=c["beta"], epoch_bounds=c["epochs"], output=output,
                       precision=None if precision == "default" else precision, max_fft_log2=c["max_fft_log2"])


IMPULSE = 8.0
OFFSET = 100.0
_CACHE = {}


def recording(name):
    """float32 (C, n), seeded, every channel different: white noise of unit spread, an impulse on the first and on the
    last sample of every epoch (a crop or a block edge one sample off moves them), and on channel 1 (where there is
    one) a constant 100 times the spread.  B4-1 / B4-5 are channels of one recording of five."""
    key = ("x", name)
    if key not in _CACHE:
        c = CASES[name]
        channels = 5 if name.startswith("B4") else c["channels"]
        rng = np.random.default_rng(5200 + sorted(CASES).index("B4-5" if name.startswith("B4") else name))
        x = rng.standard_normal((channels, c["n"]))
        for ch in range(channels):
            for a, b in epochs_of(name):
                x[ch, a] += IMPULSE * (1 + 0.5 * (ch % 5))
                x[ch, b - 1] -= IMPULSE * (1 + 0.25 * (ch % 5))
        if channels > 1:
            x[1] += OFFSET
        x = np.ascontiguousarray(x[:c["channels"]], dtype=np.float32)
        x.setflags(write=False)
        _CACHE[key] = x
    return _CACHE[key]


def oracle(name, channel):
    """complex128 (S, n): the oracle's float64 convolution of the mean-removed epochs with the literal kernels."""
    key = ("oracle", name, channel)
    if key not in _CACHE:
        c = CASES[name]
        ref = orc.cwt_complex(recording(name)[channel].astype(np.float64), FS, np.asarray(c["f"], dtype=np.float64),
                              epochs_of(name), gamma=c["gamma"], beta=c["beta"])
        ref.setflags(write=False)
        _CACHE[key] = ref
    return _CACHE[key]


def outside(name):
    """bool (n): the columns no epoch holds."""
    out = np.ones(CASES[name]["n"], bool)
    for a, b in epochs_of(name):
        out[a:b] = False
    return out


def as_output(ref, output):
    return ref if output == "complex" else np.abs(ref) if output == "amplitude" else np.abs(ref) ** 2


def kernels(name):
    """[(omega, L)] of the case's scales."""
    c = CASES[name]
    om = orc.hz_to_rad(np.asarray(c["f"], dtype=np.float64), FS)
    return list(zip(om.tolist(), [int(v) for v in orc.morse_lengths(om, c["gamma"], c["beta"])]))


# ---- full band -----------------------------------------------------------------------------------------------------
NUMPY_GAIN_MAX = 1 << 15        # P up to which exact_gain's NumPy sum (P x kept bins) is cheap


def response(name, scale, p, plan=None):
    """H of one scale on the P-point grid, complex128: decimated_model.exact_response; beyond 2^15 points the gain
    comes from the library's host evaluation of the same closed form (``plan.debug_exact_gain``)."""
    key = ("H", name, scale, p)
    if key not in _CACHE:
        c = CASES[name]
        om, length = kernels(name)[scale]
        if p <= NUMPY_GAIN_MAX or plan is None:
            g = exact_gain(2 * np.pi * np.arange(p) / p, om, length, c["gamma"], c["beta"])
        else:
            g = plan.debug_exact_gain(scale, np.arange(p), p)
        d = (length - 1) / 2 - (length - 1) // 2
        h = g * np.exp(-2j * np.pi * np.arange(p) * d / p)
        h.setflags(write=False)
        _CACHE[key] = h
    return _CACHE[key]


def fullband_row(X, h, lead, ne, single=False, crop_late=0):
    """IFFT_P(X H)[lead : lead + ne]: float64, or pocketfft in single precision on the product rounded to complex64."""
    z = X * h
    y = ifft(z.astype(np.complex64), workers=8) if single else ifft(z, workers=8)
    return y[lead + crop_late: lead + crop_late + ne]


def fullband_row_twiddle_late(X, h, lead, ne, p1):
    """Mutation (i): the inverse with the twiddle of spectrum row k1 = P1 - 1 one step on.  Row k1 (bins k1 + P1 k2)
    contributes e^(2 pi i k1 n / P) (its 4096-point transform at n mod 4096 ...); one step on in n2 multiplies that
    contribution by e^(2 pi i k1 / P)."""
    z = X * h
    only = np.zeros_like(z)
    only[p1 - 1::p1] = z[p1 - 1::p1]
    y = ifft(z, workers=8) + (np.exp(2j * np.pi * (p1 - 1) / z.size) - 1) * ifft(only, workers=8)
    return y[lead: lead + ne]


def fullband_row_dft4_swapped(X, h, lead, ne):
    """Mutation (iv), P1 = 4: output rows n1 = 1 and 3 of the 4-point column DFT exchanged (y[n2 + 4096 n1])."""
    y = ifft(X * h, workers=8).reshape(4, ROW).copy()
    y[[1, 3]] = y[[3, 1]]
    return y.reshape(-1)[lead: lead + ne]


# ---- block convolution ---------------------------------------------------------------------------------------------
def bc_response(name, scale):
    """H of one scale on the 4096-point grid of a block."""
    return response(name, scale, ROW)


def bc_blocks(e0, e1, hop):
    """Block numbers of an epoch: whole even-aligned pairs (kernels.h: BcBlocks)."""
    return np.arange((e0 // hop) & ~1, (((e1 - 1) // hop) | 1) + 1)


def bc_row(xm, epochs, hop, back, h, ramp=0, single=False, late_block=None, swap_pair=None, zero_block=None, size=ROW):
    """One scale's row by overlap-save, complex (n): block q of an epoch is the 4096 samples from q hop - back of the
    mean-removed recording ``xm`` (zero outside the epoch, faded over ``ramp`` samples at either end under
    precision = exact), transformed in float64; its samples [q hop, (q + 1) hop) inside the epoch are kept.
    ``single``: the block spectra rounded to complex64 as k_bc_forward leaves them, times the response in complex64,
    pocketfft's inverse in single precision.  Mutations, each naming (epoch index, position in the epoch's blocks):
    ``late_block`` that block's input taken one sample late, ``swap_pair`` the outputs of that block and the next
    exchanged, ``zero_block`` that block's samples left zero.  ``size``: the block's length (4096; F4x's time blocks
    of 2^14 points are the same overlap-save with the response on that grid)."""
    out = np.zeros(xm.size, dtype=np.complex64 if single else np.complex128)
    off = np.arange(size)
    win = np.ones(size)
    if ramp > 0:
        edge = np.minimum(off, size - 1 - off)
        u = (edge + 0.5) / ramp
        win = np.where(edge < ramp, u ** 3 * (10.0 + u * (6.0 * u - 15.0)), 1.0)
    hh = h.astype(np.complex64) if single else h
    for ei, (e0, e1) in enumerate(np.asarray(epochs).tolist()):
        qs = bc_blocks(e0, e1, hop)
        start = qs * hop - back
        if late_block is not None and late_block[0] == ei:
            start[late_block[1]] += 1
        idx = start[:, None] + off[None, :]
        v = np.where((idx >= e0) & (idx < e1), xm[np.clip(idx, 0, xm.size - 1)], 0.0) * win
        xb = fft(v, axis=1)
        y = ifft(xb.astype(np.complex64) * hh, axis=1) if single else ifft(xb * hh, axis=1)
        order = np.arange(qs.size)
        if swap_pair is not None and swap_pair[0] == ei:
            k = swap_pair[1]
            order[[k, k + 1]] = order[[k + 1, k]]
        for k, q in enumerate(qs.tolist()):
            lo, hi = max(q * hop, e0), min((q + 1) * hop, e1)
            if lo >= hi or (zero_block is not None and zero_block == (ei, k)):
                continue
            out[lo:hi] = y[order[k], lo - q * hop + back: hi - q * hop + back]
    return out


def launch_chunks(epochs, hop, chunk):
    """RESTATEMENT of pipeline.cpp's flush of the block convolution for a whole-recording execute: per launch batch of up
    to sixteen epochs the blocks are numbered through (``blk_first``) and launched ``chunk`` at a time.  Returns
    [(epoch index, position in the epoch's blocks)] of every block that is the FIRST of a launch after the first of its
    batch -- the blocks on a chunk seam."""
    seams, epochs = [], np.asarray(epochs).tolist()
    for b in range(0, len(epochs), SEG_BATCH):
        where = [(ei, k) for ei in range(b, min(b + SEG_BATCH, len(epochs))) for k in range(bc_blocks(*epochs[ei], hop).size)]
        seams += [where[b0] for b0 in range(chunk, len(where), chunk)]
    return seams


# ---- time domain ---------------------------------------------------------------------------------------------------
def direct_row(x32, mean, epochs, omega, length, gamma, beta, single=True, drop_tail=False, drop_end=False):
    """One time-domain scale, complex (n), the way k_direct sums it (kernels.hip): the first differences d[m] of the
    mean-removed, zero-extended epoch -- x[m] - x[m - 1] inside it, x~[0] and -x~[Ne - 1] at its ends -- times the
    running sums Psi[j] = psi[0] + .. + psi[j], j < L - 1, plus Psi[L - 1] x~[q - L + 1] (k_build_direct: summation by
    parts).  ``single``: the differences, taps, products and the accumulation in float32, as the kernel has them (taps
    in the order j = 0, 1, ..); else all in float64.  Mutations: ``drop_tail`` without the last term, ``drop_end`` without
    the difference -x~[Ne - 1] behind the epoch's last sample."""
    psi, _ = orc.morse_kernel(length, omega, gamma, beta)
    run = np.cumsum(psi)
    ft, ct = (np.float32, np.complex64) if single else (np.float64, np.complex128)
    taps, tail = run[:length - 1].astype(ct), run[length - 1].astype(ct)
    top = (length - 1) // 2
    out = np.zeros(x32.size, dtype=ct)
    for e0, e1 in np.asarray(epochs).tolist():
        ne = e1 - e0
        xe = x32[e0:e1]
        xv = (xe.astype(np.float64) - mean).astype(ft)
        d = np.zeros(ne + 1, dtype=ft)
        d[1:ne] = (xe[1:] - xe[:-1]) if single else np.diff(xe.astype(np.float64))
        d[0], d[ne] = xv[0], (0.0 if drop_end else -xv[ne - 1])
        pad = length
        dz = np.concatenate([np.zeros(pad, ft), d, np.zeros(pad, ft)])
        xz = np.concatenate([np.zeros(pad, ft), xv, np.zeros(pad + 1, ft)])
        re, im = np.zeros(ne, ft), np.zeros(ne, ft)
        for j in range(length - 1):                       # output q reads d[q + top - j]
            s = dz[pad + top - j: pad + top - j + ne]
            re += s * taps[j].real
            im += s * taps[j].imag
        if not drop_tail:
            s = xz[pad + top - (length - 1): pad + top - (length - 1) + ne]
            re += s * tail.real
            im += s * tail.imag
        out[e0:e1] = re + 1j * im
    return out


def plain_float32_row(x32, mean, epochs, omega, length, gamma, beta):
    """The same convolution as a plain float32 sum of products with the samples themselves (another operation order:
    measured and written down, not a gate)."""
    psi, _ = orc.morse_kernel(length, omega, gamma, beta)
    psi = psi.astype(np.complex64)
    out = np.zeros(x32.size, dtype=np.complex64)
    for e0, e1 in np.asarray(epochs).tolist():
        xv = (x32[e0:e1].astype(np.float64) - mean).astype(np.float32)
        full = np.convolve(xv, psi.real).astype(np.float32) + 1j * np.convolve(xv, psi.imag).astype(np.float32)
        out[e0:e1] = full[(length - 1) // 2: (length - 1) // 2 + (e1 - e0)]
    return out


# ---- one row of a case by the path its plan takes ------------------------------------------------------------------
def whole_epochs(name, plan):
    """True where the plan's segments are the case's epochs (no time blocks)."""
    return [(s[0], s[1]) for s in plan.segments()] == [tuple(b) for b in epochs_of(name).tolist()]


def group_of(plan, scale):
    for g in plan.debug_blockconv():
        if scale in g["scales"]:
            return g
    raise KeyError(scale)


def row_model(name, plan, channel, scale, single, exact=False):
    """Row ``scale`` of ``channel`` (complex, n samples) by a model of the path the plan takes for it, from the
    recording itself: float64, or the single-precision reference of that path (the module's docstring; ``exact``: the
    plan is one of precision = exact, whose blocks fade over BC_RAMP samples)."""
    c = CASES[name]
    x32 = recording(name)[channel]
    mean = float(x32.astype(np.float64).mean())
    om, length = kernels(name)[scale]
    method = int(plan.scale_info()["method"][scale])
    eb = epochs_of(name)
    if method == METHOD_DIRECT:
        return direct_row(x32, mean, eb, om, length, c["gamma"], c["beta"], single=single)
    xm = x32.astype(np.float64) - mean
    if method == METHOD_BLOCKCONV:
        g = group_of(plan, scale)
        return bc_row(xm, eb, g["hop"], g["back"], bc_response(name, scale), ramp=BC_RAMP if exact else 0, single=single)
    assert method == METHOD_FULLBAND
    if not whole_epochs(name, plan):
        # time blocks: overlap-save with the plan's FFT length, a hop of its first block and the taps behind an output
        # rounded up to 64 samples in front (any cut with room for the kernel gives the same float64 numbers, and
        # transforms of the same size in single precision)
        (a, b, p) = plan.segments()[0]
        back = ((length - 1 - (length - 1) // 2) + 63) & ~63
        hop = min(b - a, (p - back - (length - 1) // 2) & ~63)
        return bc_row(xm, eb, hop, back, response(name, scale, p, plan), single=single, size=p)
    out = np.zeros(x32.size, dtype=np.complex64 if single else np.complex128)
    for a, b, p in plan.segments():
        X = lc.spectrum(lc.segment_input(x32, a, b), p, single=single)
        out[a:b] = fullband_row(X, response(name, scale, p, plan), a & 63, b - a, single=single)
    return out


def factor(got, ref, hard, single):
    """By how much ``got`` misses the gates against ``ref``: the larger of max-error over the hard gate and rms-error
    over RMS_FACTOR times the single-precision reference's.  The GPU tests assert both, so either one catches."""
    mx, rms = lc.compare(got, ref)
    return max(mx / hard, rms / lc.rms_gate(single, ref))
