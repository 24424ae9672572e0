"""output_stride=K branch by branch (synths.hip and the strided store epilogues).  Every case names the branch it
targets, asserts through the plan's hooks (debug_levels, debug_interp, scale_info, info["n_interp"], debug_batches,
debug_graph_state) that it still reaches it, and holds the strided plan S to the contract of DESIGN.md ("Output
stride") against the same plan at K = 1, F, on the same input (_contract):

* ceil(N / K) columns; column j is recording sample K j;
* bit-equal to F[..., ::K]: every complex row, every row of a direct / block-convolution / full-band scale, every row
  of an interpolated level (k_synthis) and every row of the k_synth fallback (one kernel at both K: only its stores
  differ);
* amplitude / power rows of the k_synth7 levels (k_synth7s): within SYNTH7_TOL of the row's peak -- the complex
  values are k_synth7's, but the compiler contracts the last radix-16 layer's multiply-adds differently in the two
  kernels' |.| instantiations: up to two units in the last place of the peak on amplitude rows (measured 2.24e-7 over
  this module), twice that relative to the peak on power rows, the square (measured 3.3e-7);
* columns of samples outside every epoch: exactly 0.

k_synth7s makes a column (block, phase r) only when g = gcd(R, K) divides seg0 + r, seg0 the segment's first sample
(the epoch's, rounded down to 64); NCOL columns per workgroup, R > NCOL: one tile of NCOL phases.  Covered (the
levels as planned today; each case asserts what it needs of them):

  case                           R            g               NCOL            halo      band shift  seg0 mod 256
  phase_selection_every_g        2 .. 256     1 .. 256        32, 16          19 .. 27  0           0
  narrow_levels                  2, 4, 8      1 .. 8          16 (R <= 0/2/4) 20 .. 30  0           0
  segment_residues               8 .. 512     128, 256, 512   32              18 .. 31  0           64, 128, 192
  shifted_bands (interp off)     2 .. 64      1 .. 64         32              41 .. 75  68 .. 83    0
  deep_halo                      16           1 .. 16         32              38        0           0
  wide_halo_on_a_shifted_band    8            1 .. 8          32 (items7w)    51        66          0
  fuse_blocks_off                2 .. 256     1 .. 256        32              18 .. 32  0           0

and the k_synth fallback (halo > 48 on an unshifted band, a level of 300 scales, synth16 = 1), k_synthis (ragged
epochs, K below / at / above the interpolation factor, time blocks), precision 'fast' / 'exact', fullband4 on and
off, three batches of epochs, long mode (FFTs of 2^23), execute_block ranges, graph replay, the float64 oracle on one
small case per family and a seeded sweep of random layouts."""
import math

import numpy as np
import pytest

from oracle import ghost_oracle as orc

pytestmark = pytest.mark.gpu

TOL = 1e-5
SYNTH7_TOL = {"amplitude": 2.5e-7, "power": 5e-7}     # two last-place units of the peak (2^-22), and for the square
_WORST = {}              # output mode -> the largest k_synth7 row difference seen, relative to the row's peak


def _levels(plan):
    """Per level: decimation, halo, band shift, interpolation factor (0: not interpolated) and the plan's scales on it
    (a scale finds its level by (decimation, halo, hop): shifted bands split one decimation by halo)."""
    from ghost_amd import _lib
    si = plan.scale_info()
    lv, interp = plan.debug_levels(), plan.debug_interp()["levels"]
    keys = [(l["decimation"], l["halo"], l["hop"]) for l in lv]
    assert len(set(keys)) == len(keys), keys
    spectral = si["method"] == _lib.SCALE_SPECTRAL
    for l, i in zip(lv, interp):
        l["factor"] = i["factor"] if i is not None else 0
        l["scales"] = np.flatnonzero(spectral & (si["decimation"] == l["decimation"]) & (si["halo"] == l["halo"]) &
                                     (si["hop"] == l["hop"]))
    assert sum(l["scales"].size for l in lv) == spectral.sum()
    return [l for l in lv if l["scales"].size]


def _kernel(level, synth16=False):
    """The synthesis kernel of a level (api.cpp: level_kernel)."""
    if synth16 and level["band_shift"] == 0:
        return "k_synth"
    if level["factor"]:
        return "k_synthi"
    if level["scales"].size <= 256 and (level["halo"] <= 48 or level["band_shift"] > 0):
        return "k_synth7"
    return "k_synth"


def _signature(plan):
    return ([(l["decimation"], l["halo"], l["band_shift"], l["factor"], l["scales"].tolist()) for l in _levels(plan)],
            plan.scale_info()["method"].tolist())


def _inside(bounds, samples):
    s = np.asarray(samples)
    return np.any([(s >= a) & (s < b) for a, b in np.asarray(bounds).reshape(-1, 2)], axis=0).reshape(s.shape)


def _contract(plan, got, want, samples, msg="", synth16=False):
    """got: rows of the strided plan `plan` for the recording samples `samples` (its kept ones, in order); want: the
    K = 1 rows of the same samples."""
    from ghost_amd import _lib
    assert got.shape == want.shape and got.dtype == want.dtype, (msg, got.shape, want.shape)
    assert got.shape[-1] == len(samples), msg
    if got.shape[-1] == 0:
        return
    loose = np.zeros(got.shape[1], bool)
    if not np.iscomplexobj(got):
        for l in _levels(plan):
            if _kernel(l, synth16) == "k_synth7":
                loose[l["scales"]] = True
    np.testing.assert_array_equal(got[:, ~loose], want[:, ~loose], err_msg=str(msg))
    if loose.any():
        a, b = got[:, loose].astype(np.float64), want[:, loose].astype(np.float64)
        diff, peak = np.abs(a - b).max(axis=-1), np.abs(b).max(axis=-1)
        err = float((diff / np.where(peak > 0, peak, 1.0)).max())
        key = "power" if plan.out_mode == _lib.OUT_POWER else "amplitude"
        _WORST[key] = max(_WORST.get(key, 0.0), err)
        assert np.all(diff <= SYNTH7_TOL[key] * peak), (msg, err)
    outside = ~_inside(plan.bounds, samples)
    assert not np.any(got[..., outside]), msg


class _Layout:
    """One layout at K = 1 (F, its rows a) and, per K, the same plan at output_stride=K (S) against it."""

    def __init__(self, x, fs, f, synth16=False, **kw):
        from ghost_amd.engine import CwtPlan
        self.x = np.atleast_2d(np.asarray(x, dtype=np.float32))
        self.fs, self.f, self.kw, self.synth16 = float(fs), np.asarray(f, dtype=np.float64), kw, synth16
        self.n = self.x.shape[1]
        self.full = CwtPlan(self.n, self.x.shape[0], self.fs, self.f, **kw)
        self.a = self.full.execute(self.x)
        self.levels = _levels(self.full)
        self.bounds = self.full.bounds

    def check(self, k, ranges=()):
        """S at K = k: F's levels, the contract on execute, and execute_block over `ranges` equal to the matching
        columns of S's execute."""
        from ghost_amd.engine import CwtPlan
        s = CwtPlan(self.n, self.x.shape[0], self.fs, self.f, output_stride=k, **self.kw)
        assert _signature(s) == _signature(self.full), k
        b = s.execute(self.x)
        assert b.shape == self.a.shape[:2] + (-(-self.n // k),)
        _contract(s, b, self.a[..., ::k], np.arange(0, self.n, k), "K=%d %s" % (k, self.kw), self.synth16)
        for start, length in ranges:
            _block(s, self.x, b, k, start, length)
        s.close()
        return b

    def close(self):
        self.full.close()


def _block(plan, x, b, k, start, length):
    """execute_block(start, length) of a strided plan: the columns of the range's kept samples of its execute."""
    blk = plan.execute_block(x, start, length)
    c0, c1 = -(-start // k), -(-(start + length) // k)
    assert blk.shape[-1] == c1 - c0, (k, start, length)
    np.testing.assert_array_equal(blk, b[..., c0:c1], err_msg="K=%d block %d + %d" % (k, start, length))


def _ranges(rng, n, k, bounds, count=4):
    """`count` random ranges; one between two kept samples (no column); ranges starting one sample before and one
    after a kept sample; an epoch gap, if there is one."""
    out = []
    for _ in range(count):
        a = int(rng.integers(0, n))
        out.append((a, int(rng.integers(1, n - a + 1))))
    j = int(rng.integers(0, max(1, (n - 1) // k)))
    if k > 2 and k * j + k <= n:
        out.append((k * j + 1, k - 2))
    for s in (k * j - 1, k * j + 1):
        if 0 <= s < n:
            out.append((s, int(min(n - s, 1 + rng.integers(0, 3 * k + 2)))))
    eb = np.asarray(bounds).reshape(-1, 2)
    for (_, b0), (a1, _) in zip(eb[:-1], eb[1:]):
        if a1 - b0 >= 2:
            out.append((int(b0), int(a1 - b0)))
            break
    return out


def _lfp(c, n, fs, seed=1234):
    from ghost_amd.synthetic import lfp
    return lfp(c, n, fs, seed=seed)


def _oracle(plan, got, x, fs, f, k, output, gamma=3.0, beta=20.0):
    """Kept columns against the float64 oracle at TOL (2 TOL on power rows): a bug the full and the strided rows share
    does not pass."""
    x = np.atleast_2d(x)
    ref = np.stack([orc.cwt_complex(x[c].astype(np.float64), fs, np.asarray(f), plan.bounds, gamma=gamma, beta=beta)
                    for c in range(x.shape[0])])[..., ::k]
    if output == "amplitude":
        ref = np.abs(ref)
    elif output == "power":
        ref = np.abs(ref) ** 2
    scale = np.abs(ref).max(axis=-1, keepdims=True)
    scale[scale == 0] = 1.0
    err = (np.abs(got - ref) / scale).max()
    assert err < (2 * TOL if output == "power" else TOL), (k, output, err)


# ---- k_synth7s: phase selection ------------------------------------------------------------------------------------

PHASE_F = np.geomspace(300.0, 0.9, 32)       # 1 kHz: levels R = 2 .. 512 with the interpolating kernel off
PHASE_N = 70001


def _phase_ks(n):
    # g = gcd(R, K): 1 (3, 997, N - 1), every power of two to 256, g < R (4 on R >= 8), R | K with K != R (48 on R = 16,
    # 96 on 32, 384 and 640 on 128), K = 1000 (g = 8), N and N + 7 (one column)
    return [3, 2, 4, 8, 16, 32, 64, 128, 256, 48, 96, 384, 640, 1000, 997, n - 1, n, n + 7]


@pytest.mark.parametrize("ncol", [32, 16])
@pytest.mark.parametrize("output", ["amplitude", "power", "complex"])
def test_phase_selection_every_g(option, output, ncol):
    """k_synth7s on every level (interpolating kernel off), R = 2 .. 512, K such that g takes every power of two from
    1 to 256, NCOL = 32 and 16 (R > NCOL from R = 64, resp. R = 32: one phase tile per workgroup)."""
    option("interp", 0)
    option("synth_cols", ncol)
    lay = _Layout(_lfp(2, PHASE_N, 1000.0, seed=11), 1000.0, PHASE_F, output=output)
    rs = sorted(l["decimation"] for l in lay.levels)
    assert all(_kernel(l) == "k_synth7" and l["halo"] <= 32 and l["band_shift"] == 0 for l in lay.levels)
    assert {2, 4, 8, 16, 32, 64, 128, 256} <= set(rs), rs
    seen = set()
    for k in _phase_ks(PHASE_N):
        seen |= {math.gcd(r, k) for r in rs}
        lay.check(k)
    assert {1, 2, 4, 8, 16, 32, 64, 128, 256} <= seen, seen
    lay.close()


@pytest.mark.parametrize("narrow_r", [0, 2, 4])
def test_narrow_levels(option, narrow_r):
    """synth7_narrow_r: levels of R <= narrow_r go to the 16-column list (items7n) beside the 32-column one; 0: none."""
    option("interp", 0)
    option("synth7_narrow_r", narrow_r)
    for output in ("amplitude", "complex"):
        lay = _Layout(_lfp(2, 30001, 1000.0, seed=5), 1000.0, PHASE_F[:14], output=output)
        rs = {l["decimation"] for l in lay.levels}
        assert {2, 4, 8} <= rs and all(_kernel(l) == "k_synth7" for l in lay.levels), rs
        for k in (2, 3, 4, 6, 8, 12, 40):
            lay.check(k)
        lay.close()


def test_segment_residues(option):
    """Three epochs of one batch starting a few samples past 64, 128 and 192 (mod 256): their segments start at those
    residues, so on the levels of R >= 256 the phase test sees seg0 & (g - 1) = 64, 128 and 192 (K = 128, 256, 384,
    512); execute_block across the epochs and their gaps."""
    option("interp", 0)
    fs, n = 1000.0, 150000
    starts = [256 * 2 + 64 + 3, 256 * 200 + 128 + 5, 256 * 400 + 192 + 7]
    eb = np.array([[s, s + 45000] for s in starts])
    assert [(s & ~63) % 256 for s in starts] == [64, 128, 192]
    x = _lfp(2, n, fs, seed=21) + np.array([[0.3], [-2.0]], np.float32)
    rng = np.random.default_rng(64)
    for output in ("amplitude", "power", "complex"):
        lay = _Layout(x, fs, np.geomspace(60.0, 0.6, 12), epoch_bounds=eb, output=output)
        assert lay.full.debug_batches() == [(0, 3)]
        big = [l["decimation"] for l in lay.levels if l["decimation"] >= 256 and _kernel(l) == "k_synth7"]
        assert big, lay.levels
        residues = set()
        for k in (128, 256, 384, 512):
            for r in big:
                g = math.gcd(r, k)
                residues |= {(s & ~63) & (g - 1) for s in starts}
            lay.check(k, ranges=_ranges(rng, n, k, eb) if output == "amplitude" else ())
        assert {64, 128, 192} <= residues, residues
        lay.close()


# ---- k_synth7s: shifted bands, halos, fused blocks -----------------------------------------------------------------

@pytest.mark.parametrize("interp", [0, None])
def test_shifted_bands(option, interp):
    """Morse(3, 4): two-sided bands, every level's band shifted below zero (phase_carrier).  g >= 4 (phase-major
    columns) and g < 4; with the interpolating kernel on, its levels carry the shift too."""
    option("interp", interp)
    rng = np.random.default_rng(34)
    for output in ("amplitude", "power", "complex"):
        lay = _Layout(_lfp(2, 70001, 1000.0, seed=3), 1000.0, np.geomspace(300.0, 1.0, 20), gamma=3.0, beta=4.0,
                      output=output)
        assert lay.levels and all(l["band_shift"] > 0 for l in lay.levels)
        syn7 = {l["decimation"] for l in lay.levels if _kernel(l) == "k_synth7"}
        if interp == 0:
            assert {2, 4, 8, 16, 32, 64} <= syn7, syn7
            assert {l["halo"] > 48 for l in lay.levels} == {False, True}      # items7 and items7w
        else:
            assert syn7 and (lay.full.info["n_interp"] > 0) == (output != "complex")   # (k_synthi: |.| only)
        for k in (2, 3, 8, 64, 5, 24):
            lay.check(k, ranges=_ranges(rng, 70001, k, lay.bounds, 2) if output == "power" else ())
        lay.close()


def test_deep_halo(option):
    """Halo 33 .. 48 (a long kernel on a short recording caps R at 16; the interpolating kernel, which takes that level
    by default, off): k_synth7s tests each row's place in the block."""
    option("interp", 0)
    for output in ("amplitude", "power", "complex"):
        lay = _Layout(_lfp(2, 1500, 1000.0), 1000.0, [100.0, 10.0], output=output)
        deep = [l for l in lay.levels if 33 <= l["halo"] <= 48]
        assert deep and all(_kernel(l) == "k_synth7" for l in deep), lay.levels
        for k in (2, 3, 5, 16, 17, 1499, 1500):
            lay.check(k)
        lay.close()


WIDE_SHIFTED = dict(n=1500, f=[100.0, 8.0], gamma=3.0, beta=4.0)     # one level: R = 8, halo 51, shift 66


def test_wide_halo_on_a_shifted_band():
    """Halo > 48 on a shifted band: the items7w list -- k_synth7's WIDE instantiation at K = 1, k_synth7s at K > 1 (with
    the interpolating kernel off, test_shifted_bands has more: halos 51 .. 75 at R = 2 .. 64)."""
    w = WIDE_SHIFTED
    for output in ("amplitude", "power", "complex"):
        lay = _Layout(_lfp(2, w["n"], 1000.0, seed=8), 1000.0, w["f"], gamma=w["gamma"], beta=w["beta"], output=output)
        wide = [l for l in lay.levels if l["halo"] > 48 and l["band_shift"] > 0 and _kernel(l) == "k_synth7"]
        assert wide, lay.levels
        for k in (2, 3, 4, 7, 16, 64):
            lay.check(k)
        lay.close()


def test_fuse_blocks_off(option):
    """fuse_blocks = 0: k_synth7s reads the block spectra the block-FFT pass wrote instead of making them itself."""
    option("interp", 0)
    option("fuse_blocks", 0)
    for output in ("amplitude", "complex"):
        lay = _Layout(_lfp(2, 40001, 1000.0, seed=9), 1000.0, PHASE_F[::2], output=output)
        assert max(l["decimation"] for l in lay.levels) >= 128
        assert all(_kernel(l) == "k_synth7" for l in lay.levels)
        for k in (2, 3, 4, 64, 256, 997):
            lay.check(k)
        lay.close()


# ---- the k_synth fallback --------------------------------------------------------------------------------------------

def test_k_synth_fallback(option):
    """k_synth serves halo > 48 on an unshifted band (with the interpolating kernel off: it takes that level by
    default), levels of more than 256 scales, and every unshifted level under synth16 = 1; its rows are bit-equal
    (_contract)."""
    option("interp", 0)
    lay = _Layout(_lfp(2, 1500, 1000.0), 1000.0, [100.0, 6.0], output="amplitude")
    assert any(l["halo"] > 48 and _kernel(l) == "k_synth" for l in lay.levels), lay.levels
    for k in (2, 3, 16, 33):
        lay.check(k)
    lay.close()
    option("interp", None)
    lay = _Layout(_lfp(1, 6000, 1000.0), 1000.0, np.geomspace(68.0, 38.0, 300), output="power")
    assert any(l["scales"].size > 256 and _kernel(l) == "k_synth" for l in lay.levels)
    for k in (2, 3, 7, 64):
        lay.check(k)
    lay.close()
    option("synth16", 1)
    eb = np.array([[i * 2000 + 3, i * 2000 + 1901] for i in range(10)])
    rng = np.random.default_rng(16)
    for output in ("amplitude", "power", "complex"):
        lay = _Layout(_lfp(2, 20000, 1000.0), 1000.0, [150.0, 60.0, 25.0, 6.0], synth16=True, epoch_bounds=eb,
                      output=output)
        assert lay.levels and all(_kernel(l, True) == "k_synth" for l in lay.levels)
        for k in (2, 3, 8, 64, 2001):
            lay.check(k, ranges=_ranges(rng, 20000, k, eb, 2))
        lay.close()


# ---- k_synthis ---------------------------------------------------------------------------------------------------------

INTERP_EB = np.array([[13, 20011], [20521, 47017], [47051, 89989]])


def test_interpolated_levels_on_ragged_epochs():
    """k_synthis: three epochs with gaps, bounds multiples of neither 4 nor K; K below, at and above the interpolation
    factor I of each interpolated level; the interpolated rows bit-equal."""
    fs, n = 1000.0, 90001
    x = _lfp(2, n, fs, seed=17) + 0.5
    rng = np.random.default_rng(71)
    for output in ("amplitude", "power"):
        lay = _Layout(x, fs, np.geomspace(200.0, 2.0, 24), epoch_bounds=INTERP_EB, output=output)
        facs = sorted({l["factor"] for l in lay.levels if l["factor"]})
        assert facs and max(l["decimation"] for l in lay.levels if l["factor"]) >= 16, lay.levels
        ks = sorted({3, 5, 7, 4 * facs[-1] + 1} | set(facs) | {i - 1 for i in facs} | {i + 1 for i in facs})
        for k in ks:
            assert all(b % 4 and b % k for b in INTERP_EB.ravel()), k
            lay.check(k, ranges=_ranges(rng, n, k, INTERP_EB, 2))
        lay.close()


def test_interpolated_levels_in_time_blocks():
    """k_synthis on time blocks (max_fft_log2 = 13): each block's kept samples by their recording index."""
    fs, n = 1000.0, 60001
    x = _lfp(2, n, fs, seed=4) + 0.75
    for output in ("amplitude", "power"):
        lay = _Layout(x, fs, [300.0, 150.0, 40.0, 20.0, 12.0], output=output, max_fft_log2=13)
        assert len(lay.full.segments()) > 4 and lay.full.info["n_interp"] > 0
        for k in (2, 3, 4, 8, 9, 31, 64):
            lay.check(k)
        lay.close()


# ---- other paths -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["fast", "exact"])
def test_precision_paths(precision):
    """precision = 'fast' (float32 forward transform) and 'exact' (no decimated path: every row bit-equal)."""
    from ghost_amd import _lib
    rng = np.random.default_rng(5)
    for output in ("amplitude", "complex"):
        lay = _Layout(_lfp(2, 30001, 1000.0, seed=12), 1000.0, np.geomspace(200.0, 4.0, 10), output=output,
                      precision=precision)
        m = lay.full.scale_info()["method"]
        if precision == "exact":
            assert not (m == _lib.SCALE_SPECTRAL).any()
        else:
            assert (m == _lib.SCALE_SPECTRAL).sum() >= 6
        for k in (2, 3, 16, 100):
            lay.check(k, ranges=_ranges(rng, 30001, k, lay.bounds, 2))
        lay.close()


@pytest.mark.parametrize("fullband4", [0, 1])
def test_full_band_sets(option, fullband4):
    """Full-band scales (block convolution off, Morse(3, 2), two epochs): their strided stores, sets of four or one."""
    from ghost_amd import _lib
    option("blockconv", 0)
    option("fullband4", fullband4)
    fs, n = 1000.0, 70000
    eb = np.array([[3, 41000], [41007, n]])
    rng = np.random.default_rng(4 + fullband4)
    lay = _Layout(_lfp(2, n, fs, seed=44), fs, [9.5, 8.0, 7.0, 5.5, 4.4, 3.1, 2.2], gamma=3.0, beta=2.0,
                  epoch_bounds=eb, output="complex")
    assert (lay.full.scale_info()["method"] == _lib.SCALE_FULLBAND).all()
    for k in (2, 3, 7, 64, 4099):
        lay.check(k, ranges=_ranges(rng, n, k, eb, 2))
    lay.close()


def test_three_batches():
    """Forty epochs: three launch batches of 16, 16 and 8 segments, each with its own level grids."""
    fs, n = 1000.0, 120000
    eb = np.array([[i * 3000 + (i % 3) * 11 + 1, i * 3000 + 2000 + 37 * (i % 5)] for i in range(40)])
    x = _lfp(2, n, fs) + np.array([[0.4], [-1.1]], np.float32)
    rng = np.random.default_rng(40)
    for output in ("amplitude", "complex"):
        lay = _Layout(x, fs, [320.0, 140.0, 61.0, 33.0, 9.0], epoch_bounds=eb, output=output)
        assert lay.full.debug_batches() == [(0, 16), (16, 16), (32, 8)]
        for k in (3, 16, 64, 250):
            lay.check(k, ranges=_ranges(rng, n, k, eb, 3))
        lay.close()


def test_long_mode_rows():
    """One channel, FFTs of 2^23 points (long mode): stretches of the strided resident rows -- one across a seam
    between time blocks -- against the full-rate resident rows sliced."""
    from ghost_amd.engine import CwtPlan
    from ghost_amd.synthetic import lfp_channel
    fs, n, k = 30000.0, 18000000, 30
    f = np.array([500.0, 1.0, 0.1165])
    x = lfp_channel(n, fs, channel=5)[None]
    full = CwtPlan(n, 1, fs, f, output="amplitude")
    segs = full.segments()
    assert len(segs) >= 2 and all(s[2] == 1 << 23 for s in segs)
    strided = CwtPlan(n, 1, fs, f, output="amplitude", output_stride=k)
    assert _signature(strided) == _signature(full)
    rf = full.execute_resident(x)
    rs = strided.execute_resident(x)
    assert rs.shape == (1, 3, -(-n // k))
    for a in (0, segs[1][0] - 30001, n - 9000):
        c0, c1 = -(-a // k), -(-(a + 9000) // k)
        want = rf.to_host(start=c0 * k, stop=(c1 - 1) * k + 1)[..., ::k]
        got = rs.to_host(start=c0, stop=c1)
        _contract(strided, got, want, np.arange(c0, c1) * k, "long mode at %d" % a)
    rf.free()
    rs.free()
    full.close()
    strided.close()


# ---- graph replay, the oracle --------------------------------------------------------------------------------------------

def test_strided_device_resident_executes_replay_a_graph(option):
    """A small strided device-resident plan run six times (1 eager, 2 captured, 3 .. 6 replayed) with new samples
    through the same pointers: the replay is in use and bit-equal to an eager strided plan."""
    from ghost_amd.engine import CwtPlan, DeviceBuffer
    fs, n, C, k = 1000.0, 16384, 2, 3
    f = 200.0 / 2.0 ** (np.arange(32) / 6.0)
    eb = np.array([[0, 9000], [9003, n]])
    xs = [_lfp(C, n, fs, seed=s) for s in (1, 2, 3)]
    option("graphs", 0)
    p0 = CwtPlan(n, C, fs, f, epoch_bounds=eb, output="amplitude", output_stride=k)
    eager = [p0.execute(x) for x in xs]
    option("graphs", None)
    p = CwtPlan(n, C, fs, f, epoch_bounds=eb, output="amplitude", output_stride=k)
    cols = -(-n // k)
    xb, ob = DeviceBuffer(4 * C * n), DeviceBuffer(p.info["out_bytes"])
    for _ in range(2):
        for x, want in zip(xs, eager):
            xb.upload(x)
            p.execute_device(xb, ob)
            np.testing.assert_array_equal(ob.download((C, 32, cols), np.float32), want)
    assert p.debug_graph_state() == 1 and p0.debug_graph_state() == 0
    full = CwtPlan(n, C, fs, f, epoch_bounds=eb, output="amplitude")
    _contract(p, eager[2], full.execute(xs[2])[..., ::k], np.arange(0, n, k))
    xb.free()
    ob.free()


@pytest.mark.parametrize("family", ["synth7", "shifted", "interp", "fallback", "direct", "blockconv", "fullband"])
def test_kept_columns_meet_the_oracle(option, family):
    """One small case per family: the kept columns against the float64 oracle."""
    from ghost_amd import _lib
    from ghost_amd.engine import CwtPlan
    fs, gb, eb = 1000.0, dict(gamma=3.0, beta=20.0), None
    if family == "synth7":
        option("interp", 0)
        n, f, k, output = 12001, np.geomspace(300.0, 4.0, 8), 12, "amplitude"
    elif family == "shifted":
        n, f, k, output, gb = 12001, np.geomspace(300.0, 4.0, 8), 5, "complex", dict(gamma=3.0, beta=4.0)
    elif family == "interp":
        n, f, k, output = 20011, np.geomspace(100.0, 3.0, 6), 7, "power"
        eb = np.array([[5, 9001], [9017, 20003]])
    elif family == "fallback":
        option("interp", 0)
        n, f, k, output = 1500, [100.0, 6.0], 3, "complex"
    elif family == "direct":
        n, f, k, output, gb = 8001, [300.0, 200.0, 100.0], 4, "complex", dict(gamma=1.0, beta=5.0)
    elif family == "blockconv":
        n, f, k, output, gb = 12001, [40.0, 20.0, 9.0], 6, "amplitude", dict(gamma=3.0, beta=2.0)
    else:
        option("blockconv", 0)
        n, f, k, output, gb = 12001, [4.4, 2.2], 9, "complex", dict(gamma=3.0, beta=2.0)
    x = _lfp(1, n, fs, seed=99)
    p = CwtPlan(n, 1, fs, f, epoch_bounds=eb, output=output, output_stride=k, **gb)
    m, lv = p.scale_info()["method"], _levels(p)
    reaches = {"synth7": lambda: any(_kernel(l) == "k_synth7" for l in lv),
               "shifted": lambda: any(l["band_shift"] > 0 for l in lv),
               "interp": lambda: p.info["n_interp"] > 0,
               "fallback": lambda: any(_kernel(l) == "k_synth" for l in lv),
               "direct": lambda: (m == _lib.SCALE_DIRECT).any(),
               "blockconv": lambda: (m == _lib.SCALE_BLOCKCONV).any(),
               "fullband": lambda: (m == _lib.SCALE_FULLBAND).any()}[family]
    assert reaches(), (family, m, lv)
    _oracle(p, p.execute(x), x, fs, f, k, output, **gb)
    p.close()


# ---- a seeded sweep ------------------------------------------------------------------------------------------------------

SWEEP_PAIRS = [(3.0, 8.0), (3.0, 4.0), (1.0, 5.0), (3.0, 2.0), (3.0, 5.0)]      # G11's and G15's Morse pairs


def _sweep_stride(rng, n):
    kind = int(rng.integers(0, 4))
    if kind == 0:
        return 1 << int(rng.integers(1, 10))                               # a power of two
    if kind == 1:
        return int(rng.choice([3, 5, 7, 9])) << int(rng.integers(1, 8))    # a multiple of one
    if kind == 2:
        return 2 * int(rng.integers(1, 600)) + 1                           # odd
    return int(rng.choice([max(2, n - 1), max(2, n), n + 3]))


def test_seeded_sweep():
    """Fifty random layouts (seed 355): 1 - 3 channels, 17 .. 150 000 samples, epochs with gaps starting a few samples
    past 64 mod 128, the G11 / G15 Morse pairs, all three outputs, K a power of two, a multiple of one or odd;
    strided against full sliced, and random execute_block ranges.  A layout the planner refuses is refused alike at
    K = 1 and K > 1."""
    from ghost_amd.engine import CwtPlan
    rng = np.random.default_rng(355)
    fs = 1000.0
    ran = 0
    for case in range(50):
        n_ch = int(rng.integers(1, 4))
        n = int(np.exp(rng.uniform(np.log(17), np.log(150000))))
        eb = None
        if n > 400 and rng.random() < 0.6:
            slots = max(1, n // 128 - 1)
            starts = np.sort(rng.choice(slots, size=min(int(rng.integers(1, 5)), slots), replace=False)) * 128 + 64
            starts = starts + rng.integers(0, 4, size=starts.size)
            ends = list(starts[1:] - rng.integers(0, 40, size=starts.size - 1)) + [n - int(rng.integers(0, 5))]
            eb = np.array([[a, b] for a, b in zip(starts, ends) if b - a > 8]).reshape(-1, 2)
            if eb.shape[0] == 0:
                eb = None
        gamma, beta = SWEEP_PAIRS[int(rng.integers(0, len(SWEEP_PAIRS)))]
        span = n if eb is None else int((eb[:, 1] - eb[:, 0]).min())
        lo, hi = max(0.5, 6.0 * fs / span), 0.4 * fs
        ns = int(rng.integers(1, 7))
        f = np.sort(np.exp(rng.uniform(np.log(lo), np.log(hi), ns)))[::-1] if lo < hi else np.array([hi])
        output = ["complex", "amplitude", "power"][int(rng.integers(0, 3))]
        k = _sweep_stride(rng, n)
        x = (rng.standard_normal((n_ch, n)) + 0.05 * np.cumsum(rng.standard_normal((n_ch, n)), axis=1)
             + rng.uniform(-3, 3, (n_ch, 1))).astype(np.float32)
        kw = dict(gamma=gamma, beta=beta, epoch_bounds=eb, output=output)
        try:
            lay = _Layout(x, fs, f, **kw)
        except Exception as e:
            with pytest.raises(type(e)) as again:
                CwtPlan(n, n_ch, fs, f, output_stride=k, **kw).execute(x)
            assert str(again.value) == str(e), (case, str(e))
            continue
        lay.check(k, ranges=_ranges(rng, n, k, lay.bounds, 2))
        lay.close()
        ran += 1
    assert ran >= 35, ran
