"""Shared pieces of the front-end tests (plain module, no fixtures, no GPU): the cases that between them reach every
kernel between the recording and x_R -- the forward transform in float64 (csrc/fwd64.hip) and float32 (csrc/kernels.hip),
the band gather, the per-level inverse row and column passes, k_level_small -- and the block spectra; a restatement of
the dispatch that picks those kernels; seeded recordings; float64 models of every stage and the single-precision
reference the gates are taken from (tests/test_level_cases_cpu.py pins the planner's decisions and shows what the
comparison catches, tests/test_gpu_level_matrix.py runs the cases; profiles/level_matrix.md has the measurements).

Case  plan (1 kHz unless said)                                 what it is there for
1     n = 2000, geomspace(200, 20, 8)                          P = 2^12, P1 = 1: no level column pass, tw_n = 0; rows of
                                                               2048 .. 256
2     n = 20000, geomspace(200, 0.6, 24)                       P = 2^16, P1 = 16: every row length 2048 .. 16 (k_fft_rows_fast
                                                               down to 256, k_fft_rows below), generic columns
3     n = 140000, geomspace(200, 0.086, 24)                    P = 2^19, P1 = 128: the largest generic column pass;
                                                               k_level_small at R = 512, 1024, 2048, all q > 1
4     n = 270000, geomspace(200, 0.05, 24)                     P = 2^20, P1 = 256: k_fft_cols256<+1>; k_level_small down to
                                                               M = 256 (q = 1)
5     n = 1000000, the same grid                               P = 2^21, P1 = 512: k_fft_colsq<+1,false,1>
6     n = 2100000, the same grid                               P = 2^22, P1 = 1024: k_fft_colsq<+1,false,2>; k_level_small
                                                               at M = 8192, n1 = 1024, q = 8 (64 KB of LDS: its limit)
7     n = 20000, Morse(3, 4), geomspace(100, 2, 12)            band_shift 66 .. 71, two levels sharing R = 2, P1 = 8
8     n = 270000, Morse(3, 4), geomspace(100, 0.5, 12)         P1 = 128, shifts 57 .. 88, three pairs of levels sharing R
9     n = 1000000, Morse(3, 4), geomspace(100, 0.1, 24)        a full-band scale: every row of the spectrum is built,
                                                               none mirrored, 4096 bins of each stored; shifted levels
9s    n = 500000, the same grid, precision = 'fast' only       the same at P1 = 256: k_fft_cols256<-1,true>
10    n = 38400, six epochs [6400 i, 6400 i + 5000 + i % 3)    one launch batch of six segments, P1 = 2
10L   the same, starts 6400 i + 7 + 5 i                        the same with a lead of 7 .. 32 zeros per segment
11    30 kHz, n = 2^20, [1000, 60, 0.13]                       long mode: P = 2^23 as A = 2 interleaved transforms; a
                                                               two-pass level of either row kernel and k_level_small

Cases 1, 4, 5, 6, 9 also run with precision = 'fast' (no low cut, the float32 forward kernels); 2 and 4 also with option
slow_fft = 1 (the generic kernels at every size).

Not reached by any plan: k_fft_colsq<-1,true,1|2>.  launch_fft_cols_segs takes them for real input only when a segment
of the batch has no valid sample, and pipeline.cpp never puts such a segment into a batch (n_valid is the segment's ne > 0;
segments with nothing to write are skipped before).  ``forward_kernels`` names them for ``all_nonempty=False``."""
import numpy as np
from scipy.fft import fft, ifft

from decimated_model import low_cut

ROW = 4096                      # kernels.h: kRowLen, bins per row of the stored spectrum
BLOCK = 256                     # B
MAX_TWO_PASS = 256              # planner.h: kMaxTwoPassDecimation
STORE_LOG2 = 22                 # planner.h: a stored spectrum has at most 2^22 bins

# The project's own gates (tests/test_gpu_stages.py: test_forward_decimate_block_stages), max|err| / max|ref|
GATE_SPECTRUM = 2e-6
GATE_XR = 3e-6
GATE_BLOCKS = 3e-6
GATE_ROWS = 1e-5                # final rows, conftest.rel_err (the oracle gate)
# rms(err) / rms(ref) of a stage may be RMS_FACTOR times that of the same transform made by scipy.fft on complex64
# data (pocketfft in single precision) against float64: the kernels use table twiddles and two or three radix-2 /
# radix-16 passes with one more twiddle rounding each, pocketfft fewer.  No variant has needed a factor of its own.
RMS_FACTOR = 4.0
CAUGHT = 10.0                   # a mutation of the model must exceed a gate by this factor

_G = np.geomspace
_EPOCHS10 = [[6400 * i, 6400 * i + 5000 + i % 3] for i in range(6)]
_EPOCHS10L = [[6400 * i + 7 + 5 * i, 6400 * i + 7 + 5 * i + 5000 + i % 3] for i in range(6)]

CASES = {
    "1": dict(n=2000, fs=1000.0, f=_G(200.0, 20.0, 8), gamma=3.0, beta=20.0, epochs=None, channels=3,
              precisions=("default", "fast"), why="P1 = 1: no column pass, rows 2048 .. 256"),
    "2": dict(n=20000, fs=1000.0, f=_G(200.0, 0.6, 24), gamma=3.0, beta=20.0, epochs=None, channels=3,
              precisions=("default",), why="every row length 2048 .. 16, generic columns"),
    "3": dict(n=140000, fs=1000.0, f=_G(200.0, 0.086, 24), gamma=3.0, beta=20.0, epochs=None, channels=3,
              precisions=("default",), why="P1 = 128, k_level_small with q > 1"),
    "4": dict(n=270000, fs=1000.0, f=_G(200.0, 0.05, 24), gamma=3.0, beta=20.0, epochs=None, channels=2,
              precisions=("default", "fast"), why="P1 = 256, k_level_small with q = 1"),
    "5": dict(n=1000000, fs=1000.0, f=_G(200.0, 0.05, 24), gamma=3.0, beta=20.0, epochs=None, channels=2,
              precisions=("default", "fast"), why="P1 = 512"),
    "6": dict(n=2100000, fs=1000.0, f=_G(200.0, 0.05, 24), gamma=3.0, beta=20.0, epochs=None, channels=2,
              precisions=("default", "fast"), why="P1 = 1024, k_level_small at its LDS limit"),
    "7": dict(n=20000, fs=1000.0, f=_G(100.0, 2.0, 12), gamma=3.0, beta=4.0, epochs=None, channels=3,
              precisions=("default",), why="shifted bands, two levels sharing R = 2"),
    "8": dict(n=270000, fs=1000.0, f=_G(100.0, 0.5, 12), gamma=3.0, beta=4.0, epochs=None, channels=2,
              precisions=("default",), why="shifted bands at P1 = 128, three shared decimations"),
    "9": dict(n=1000000, fs=1000.0, f=_G(100.0, 0.1, 24), gamma=3.0, beta=4.0, epochs=None, channels=2,
              precisions=("default", "fast"), why="a full-band scale: the whole spectrum, nothing mirrored"),
    "9s": dict(n=500000, fs=1000.0, f=_G(100.0, 0.1, 24), gamma=3.0, beta=4.0, epochs=None, channels=2,
               precisions=("fast",), why="the same at P1 = 256 in float32"),
    "10": dict(n=38400, fs=1000.0, f=_G(200.0, 10.0, 8), gamma=3.0, beta=20.0, epochs=_EPOCHS10, channels=3,
               precisions=("default",), why="a batch of six segments"),
    "10L": dict(n=38400, fs=1000.0, f=_G(200.0, 10.0, 8), gamma=3.0, beta=20.0, epochs=_EPOCHS10L, channels=3,
                precisions=("default",), why="a batch of six segments with leads"),
    "11": dict(n=1 << 20, fs=30000.0, f=np.array([1000.0, 60.0, 0.13]), gamma=3.0, beta=20.0, epochs=None, channels=2,
               precisions=("default",), why="long mode, A = 2"),
}
SLOW_FFT_CASES = ("2", "4")                   # also run with option slow_fft = 1
STREAM_CASES = ("3", "8")                     # level_streams = 0 must give the bits of the default plan
BLOCK_CASES = ("1", "2", "7", "10")           # block spectra are fetched (P <= 2^16)
DEFAULT_SPECTRUM_CASES = ("9", "10", "10L", "11")   # the float64 forward spectrum is compared here too
RUNS = [(name, prec) for name, c in CASES.items() for prec in c["precisions"]]

# What the planner decides, per case (default precision; 9s: fast): FFT length, P1 of the stored spectrum, A,
# (decimation, band_shift) per level, launch batches, methods
EXPECT = {
    "1": dict(p=1 << 12, p1=1, a=1, levels=[(2, 0), (4, 0), (8, 0), (16, 0)], batches=[(0, 1)], methods={0}),
    "2": dict(p=1 << 16, p1=16, a=1, levels=[(1 << k, 0) for k in range(1, 9)], batches=[(0, 1)], methods={0}),
    "3": dict(p=1 << 19, p1=128, a=1, levels=[(2, 0)] + [(1 << k, 0) for k in range(3, 12)], batches=[(0, 1)], methods={0}),
    "4": dict(p=1 << 20, p1=256, a=1, levels=[(2, 0)] + [(1 << k, 0) for k in range(3, 13)], batches=[(0, 1)], methods={0}),
    "5": dict(p=1 << 21, p1=512, a=1, levels=[(2, 0)] + [(1 << k, 0) for k in range(3, 13)], batches=[(0, 1)], methods={0}),
    "6": dict(p=1 << 22, p1=1024, a=1, levels=[(2, 0)] + [(1 << k, 0) for k in range(3, 13)], batches=[(0, 1)], methods={0}),
    "7": dict(p=1 << 15, p1=8, a=1, levels=[(2, 71), (2, 71), (4, 70), (8, 69), (16, 67), (32, 66)], batches=[(0, 1)],
              methods={0, 3}),
    "8": dict(p=1 << 19, p1=128, a=1, levels=[(2, 79), (2, 79), (4, 60), (8, 74), (8, 74), (16, 57), (32, 70), (64, 88),
                                              (64, 88), (128, 72)], batches=[(0, 1)], methods={0, 3}),
    "9": dict(p=1 << 21, p1=512, a=1, levels=[(2, 84), (2, 84), (4, 68), (8, 75), (8, 75), (16, 82), (16, 82), (32, 68),
                                              (64, 76), (64, 76), (128, 80), (128, 80), (256, 80)], batches=[(0, 1)],
              methods={0, 2, 3}),
    "9s": dict(p=1 << 20, p1=256, a=1, levels=[(2, 84), (2, 84), (4, 68), (4, 68), (8, 75), (8, 75), (16, 82), (16, 82),
                                               (32, 68), (64, 76), (64, 76), (128, 80), (128, 80), (256, 80)],
               batches=[(0, 1)], methods={0, 2, 3}),
    "10": dict(p=1 << 13, p1=2, a=1, levels=[(2, 0), (4, 0), (16, 0), (32, 0)], batches=[(0, 6)], methods={0}),
    "10L": dict(p=1 << 13, p1=2, a=1, levels=[(2, 0), (4, 0), (16, 0), (32, 0)], batches=[(0, 6)], methods={0}),
    "11": dict(p=1 << 23, p1=1024, a=2, levels=[(16, 0), (256, 0), (16384, 0)], batches=[(0, 1)], methods={0}),
}


# ---- the dispatch, restated ----------------------------------------------------------------------------------------
def _cols_name(sign, real_in, length, slow_fft):
    """launch_fft_cols_segs (csrc/kernels.hip) past its two-real-columns branches."""
    tag = "%+d,%s" % (sign, "true" if real_in else "false")
    if not slow_fft and length in (512, 1024):
        return "k_fft_colsq<%s,%d>" % (tag, 1 if length == 512 else 2)
    if not slow_fft and length == 256:
        return "k_fft_cols256<%s>" % tag
    return "k_fft_cols<%s>" % tag


def level_kernels(p1, decimation, long_a=1, band_shift=0, slow_fft=False):
    """RESTATEMENT of the level branch of pipeline.cpp's level_pass ("lp.decimation / A <= kMaxTwoPassDecimation") with
    launch_fft_rows and launch_fft_cols_segs of csrc/kernels.hip: the kernels that make x_R of one level from the stored
    spectrum of p1 rows, in launch order.  A change to that dispatch must change this too."""
    r = decimation // long_a                      # decimation of the STORED spectrum
    if r > MAX_TWO_PASS:
        m = p1 * ROW // r
        n1 = min(p1, m)
        return ["k_level_small[q=1]" if m // n1 == 1 else "k_level_small[q>1]"]
    q = ROW // r
    names = ["k_shift_gather"] if band_shift > 0 else []
    names.append("k_fft_rows_fast<+1>" if q >= 256 and not slow_fft else "k_fft_rows<+1>")
    if p1 > 1:
        names.append(_cols_name(+1, False, p1, slow_fft))
    return names


def hermitian(p1, fullband, slow_fft=False):
    """pipeline.cpp: rows 0 .. P1/2 of the spectrum are built and the others written as their reflections."""
    return (not slow_fft) and p1 >= 4 and not fullband


def forward_kernels(p1, fast_precision, herm, all_nonempty=True, slow_fft=False, fullband=False):
    """RESTATEMENT of the forward transform's dispatch: launch_fwd64_cols / launch_fwd64_rows (csrc/fwd64.hip) under the
    default precision, launch_fft_cols_segs / launch_fft_rows (csrc/kernels.hip) under precision = 'fast' and, whatever
    the precision, under option slow_fft (the float64 transform has no generic form; the low cut stays).  The row
    pass is named with the form of its output: [mirror] rows 0 .. P1/2 computed and reflected into the others, [half]
    every row computed, 2048 bins of each stored, [full] every row, all 4096 bins (a plan with a full-band scale)."""
    assert not (herm and (fullband or slow_fft or p1 < 4))
    form = "[mirror]" if herm else ("[full]" if fullband else "[half]")
    if not fast_precision and not slow_fft:       # (api.cpp allocates the float64 intermediate only for the fast FFTs)
        cols = {256: "k_fwd64_cols256_real2", 512: "k_fwd64_colsq_real2<1>", 1024: "k_fwd64_colsq_real2<2>"}.get(
            p1, "k_fwd64_cols_small")
        return [cols, "k_fwd64_rows" + form]
    rows_out = p1 // 2 + 1 if herm else p1
    if p1 == 256 and not slow_fft and rows_out == 129 and all_nonempty:
        cols = "k_fft_cols256_real2"
    elif p1 in (512, 1024) and not slow_fft and all_nonempty:
        cols = "k_fft_colsq_real2<%d>" % (1 if p1 == 512 else 2)
    else:
        cols = _cols_name(-1, True, p1, slow_fft)
    # (the generic row kernel has neither an output length nor a mirror: it writes every bin of every row)
    return [cols, "k_fft_rows<-1>" if slow_fft else "k_fft_rows_fast<-1>" + form]


UNREACHABLE = {"k_fft_colsq<-1,true,1>", "k_fft_colsq<-1,true,2>"}      # (the module's docstring says why)


def all_kernel_names():
    """Every name the two functions above can return for a plan the planner can make."""
    names = set()
    for lg in range(11):
        p1 = 1 << lg
        for slow in (False, True):
            for fast in (False, True):
                for fullband in (False, True):
                    for nonempty in (True, False):
                        names.update(forward_kernels(p1, fast, hermitian(p1, fullband, slow), nonempty, slow, fullband))
            for lr in range(1, 15):
                if p1 * ROW >> lr < BLOCK:
                    continue
                for shift in (0, 1):
                    names.update(level_kernels(p1, 1 << lr, 1, shift, slow))
    return names


def reached(plan, fast_precision, slow_fft=False):
    """The kernel names one run of ``plan`` takes."""
    p = plan.segments()[0][2]
    a = max(1, p >> STORE_LOG2)
    p1 = p // a // ROW
    fullband = 2 in set(plan.scale_info()["method"].tolist())
    names = set(forward_kernels(p1, fast_precision, hermitian(p1, fullband, slow_fft), True, slow_fft, fullband))
    for lv in plan.debug_levels():
        names.update(level_kernels(p1, lv["decimation"], a, lv["band_shift"], slow_fft))
    return names


# ---- plans and recordings ------------------------------------------------------------------------------------------
def epochs_of(name):
    c = CASES[name]
    return np.array([[0, c["n"]]] if c["epochs"] is None else c["epochs"], dtype=np.int64)


def make_plan(name, precision="default", n_channels=None, output="complex"):
    from ghost_amd.engine import CwtPlan
    c = CASES[name]
    return CwtPlan(c["n"], c["channels"] if n_channels is None else n_channels, c["fs"], c["f"], gamma=c["gamma"],
                   beta=c["beta"], epoch_bounds=c["epochs"], output=output,
                   precision=None if precision == "default" else precision)


def geometry(plan):
    """(P, P_store, P1, A, stored bins per row) of a plan whose segments share one FFT length."""
    segs = plan.segments()
    p = segs[0][2]
    assert all(s[2] == p for s in segs)
    a = max(1, p >> STORE_LOG2)
    fullband = 2 in set(plan.scale_info()["method"].tolist())
    return p, p // a, p // a // ROW, a, ROW if fullband else ROW // 2


TONE = 8.0                      # amplitude of the level tones, in spreads of the noise
TONE_ALONE = 1.0                # of the one tone of a float32 case without tapered levels (tone_angles)
IMPULSE = 8.0
OFFSET = 100.0
_CACHE = {}


def tapered_levels(name):
    """How many levels of the case's default plan have a low cut."""
    return sum(lv["low_cut"] > 0 for lv in make_plan(name, n_channels=1).debug_levels())


def tone_angles(name):
    """Radians per sample of one tone per tapered level of the case's default plan: the middle of the level's low cut,
    0.75 low_cut (the cut is half a cosine from low_cut / 2 to low_cut), where the taper's slope is largest.  A case
    that runs in float32 and has no tapered level (9, 9s) gets one tone at its first scale's frequency instead: casting
    x - mean to float32 rounds the samples of the channel with the offset all the same way (they lie on the grid of
    float32 near 100), which leaves up to N ulp / 2 in the DC bin -- 7e-6 of the largest bin of plain noise at N = 10^6,
    above the spectrum's gate for pocketfft in single precision as for any float32 transform; a tone's bin is N / 2
    times its amplitude, and one spread (TONE_ALONE) keeps that bias twenty times below the gate at N = 5 10^5.  Not
    more: a float32 transform's rounding floor follows its largest bin, and x_R of the levels that do not hold the tone
    is measured against that floor end to end."""
    key = ("tones", name)
    if key not in _CACHE:
        c = CASES[name]
        angles = [0.75 * lv["low_cut"] for lv in make_plan(name, n_channels=1).debug_levels() if lv["low_cut"] > 0]
        if not angles and "fast" in c["precisions"]:
            angles = [2 * np.pi * float(c["f"][0]) / c["fs"]]
        _CACHE[key] = angles
    return _CACHE[key]


def recording(name):
    """float32 (C, n), seeded, every channel different: white noise of unit spread (every bin of the spectrum and every
    sample of x_R of comparable size), one tone per level in the middle of that level's low cut (a taper one bin off
    moves the level's x_R at first order), an impulse on the first and on the last valid sample of every segment, and on
    channel 1 a constant 100 times the spread."""
    key = ("x", name)
    if key not in _CACHE:
        c = CASES[name]
        seed = sorted(CASES).index(name)
        rng = np.random.default_rng(4100 + seed)
        x = rng.standard_normal((c["channels"], c["n"]))
        t = np.arange(c["n"], dtype=np.float64)
        amplitude = TONE if tapered_levels(name) else TONE_ALONE
        for ch in range(c["channels"]):
            for l, th in enumerate(tone_angles(name)):
                x[ch] += amplitude * (1 + 0.25 * ch) * np.cos(th * t + 0.7 * l + 1.3 * ch)
            for a, b in epochs_of(name):
                x[ch, a] += IMPULSE * (1 + ch)
                x[ch, b - 1] -= IMPULSE * (1 + 0.5 * ch)
        x[1] += OFFSET
        x = np.ascontiguousarray(x, dtype=np.float32)
        x.setflags(write=False)
        _CACHE[key] = x
    return _CACHE[key]


def segment_input(x_channel, start, stop):
    """float64: what the forward transform of one segment reads -- the channel minus its mean over the whole recording,
    samples [start, stop), after the zeros that bring the segment's start down to a multiple of 64."""
    x = np.asarray(x_channel, dtype=np.float64)
    lead = int(start) & 63
    return np.concatenate([np.zeros(lead), x[start:stop] - x.mean()])


# ---- the float64 models --------------------------------------------------------------------------------------------
def spectrum(seg, p, single=False):
    """X (P bins, natural order) of a segment's input: float64, or pocketfft in single precision."""
    v = np.zeros(p, dtype=np.complex64 if single else np.complex128)
    v[:seg.size] = seg
    return fft(v, workers=8)


def stored(X, p1, ncol):
    """The stored spectrum of a natural-order one, k1-major: S[k1][k2] = X[k1 + P1 k2], k2 < ncol.  Long mode stores
    exactly these bins of the TRUE spectrum, with P1 = 1024 (planner.h: EpochPlan::long_a)."""
    return X[:p1 * ncol].reshape(ncol, p1).T


def natural(S):
    """The low bins X[0 .. P1 ncol) of a stored spectrum (P1, ncol), natural order."""
    return np.ascontiguousarray(S.T).reshape(-1)


def level_slice(xlo, p, lv, shift_bins=None, taper_roll=0):
    """The M bins one level transforms, from the spectrum's low bins ``xlo`` (X[k], k >= 0; the recording is real, so
    X[-k] = conj X[k]): bins -U .. M - U - 1 with U = band_shift M / 256, times the level's low cut.  ``shift_bins``
    overrides U, ``taper_roll`` moves the cut by that many bins (the CPU tests' mutations)."""
    m = int(lv["m"])
    u = lv["band_shift"] * m // BLOCK if shift_bins is None else shift_bins
    k = np.arange(m) - u
    sl = np.where(k >= 0, xlo[np.abs(k)], np.conj(xlo[np.abs(k)]))
    return sl * np.roll(low_cut(lv["low_cut"], p, m), taper_roll)


def xr_of_slice(sl, single=False):
    """x_R = IFFT_M(slice) M: the unnormalised inverse, as the level passes leave it (P x_lp[R m])."""
    if single:
        return ifft(sl.astype(np.complex64), workers=8) * np.float32(sl.size)
    return ifft(sl, workers=8) * sl.size


def xr_model(xlo, p, lv):
    return xr_of_slice(level_slice(xlo, p, lv))


def block_index(lv):
    """(nblk, 256) indices into x_R of every block of a level (circular)."""
    return ((np.arange(lv["nblk"])[:, None] * lv["hop"] - lv["halo"] + np.arange(BLOCK)[None, :]) % lv["m"])


def blocks_model(xr, p, lv, single=False, late_block=None):
    """Every block spectrum of a level, (nblk, 256): FFT_256(x_R[b hop - halo + (0 .. 255)]) / (256 P).  ``late_block``:
    that block taken one sample late (a mutation)."""
    idx = block_index(lv)
    if late_block is not None:
        idx[late_block] = (idx[late_block] + 1) % lv["m"]
    v = xr[idx]
    if single:
        return fft(v.astype(np.complex64), axis=1) * np.float32(1.0 / (BLOCK * float(p)))
    return fft(v, axis=1) / (BLOCK * float(p))


def row_contribution(sl, p1, j1):
    """What row j1 of the k1-major slice (bins j1 + P1 j2) adds to x_R.  The two-pass inverse makes x_R[Q m1 + m2] =
    sum_j1 e^(2 pi i j1 m1 / P1) e^(2 pi i j1 m2 / M) (row j1's transform at m2); advancing the twiddle of row j1 one
    step (m2 + 1 for m2) multiplies this contribution by e^(2 pi i j1 / M)."""
    only = np.zeros_like(sl)
    only[j1::p1] = sl[j1::p1]
    return ifft(only, workers=8) * sl.size


def compare(got, ref):
    """(max|err| / max|ref|, rms(err) / rms(ref))."""
    got, ref = np.asarray(got), np.asarray(ref)
    err = np.abs(got.astype(np.complex128) - ref).ravel()
    mag = np.abs(ref).ravel()
    return float(err.max() / mag.max()), float(np.sqrt(np.mean(err ** 2) / np.mean(mag ** 2)))


def rms_gate(single, ref):
    """The tighter gate of a stage: RMS_FACTOR times rms(err) / rms(ref) of the single-precision reference."""
    return RMS_FACTOR * compare(single, ref)[1]
