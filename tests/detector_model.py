"""Float64 model of the precision detector's predictions (csrc/detect.hip: k_precision_predict), the cases the detector
tests run and the bound they hold the kernel to (test helper; no GPU, no fixtures).

DESIGN.md section 3 ('auto'): from the spectrum's band energies h_b, sixteen bands per octave of the bin index, two
predicted losses per scale relative to the scale's own output.  Per level with decimation R on an FFT of P points:
top = P / R bins, per_bin = top / 256 spectrum bins per bin of the level's 256-point grid, U = shift per_bin bins of it
below zero frequency.

  w_b        fraction of band b inside [0, top - U), plus the fraction inside [0, U) on a shifted level (the mirrored
             copy), times t^2 under a low cut: t half a cosine of the band's centre between k0 = k1 / 2 and
             k1 = low_cut P / 2 pi (only when the level whose x_R is read is unshifted and k1 - k0 >= 1)
  E_level    sum_b w_b h_b: what the level's float32 stages see
  out_b      (1 - min(w_b, 1)) h_b: what the level leaves out of band b
  d_j        density of grid bin j: h_b / max(1, width_b) per_bin for the band b of |(j - shift + 1/2) per_bin|, at least 1
  E_s        sum_j d_j min{G_i^2 : i on j's side of zero frequency, band(i) = band(j)}
  W_s        sum_j G_j^2 / 256
  E_out      sum_b r_b^2 out_b, r_b = min(1, 2 L c_b / P) for bands centred at c_b < top on an unshifted level, else 1
  rounding   kappa sqrt(E_level W_s / E_s);  left_out = oob sqrt(E_out / E_s);  both 0 when E_s = 0
  predicted  max(rounding, left_out); 0 for scales off the decimated path

G_j is the scale's gain at grid bin j, theta = 2 pi (j - shift) / (256 R) (kernels.hip: k_build_bank counts the bins
from the bottom of the level's band), rounded to the float32 the table holds.  ``predict`` takes switches that damage
the model on purpose: tests/test_detector_cases_cpu.py shows with them that the comparison sees such errors."""
import numpy as np
from scipy.fft import fft

from decimated_model import level_of_scale

N_BANDS = 16 * 24
GRID = 256
KAPPA, OOB, THRESHOLD = 1.6e-7, 2.5e-8, 1.5e-6          # options auto_kappa_ppb, auto_oob_ppt, auto_threshold_ppb
FS = 1000.0

# The bound (profiles/detector_model.md): every sum has at most 384 non-negative float32 terms (388 * 2^-24 = 2.3e-5
# whatever the order); a term is the root of a product and quotient of three of them; 1 - w carries the absolute error
# of float32 weights and of __cosf inside a cut's transition.
REL_TOL = 1e-4
ABS_WEIGHT = 2e-6
MARGIN = 0.02                                            # no prediction of a case this close to the threshold

_B = np.arange(N_BANDS)
BAND_LO = np.ldexp(1.0 + (_B & 15) / 16.0, _B >> 4)
BAND_HI = np.ldexp(1.0 + ((_B & 15) + 1) / 16.0, _B >> 4)
BAND_MID = 0.5 * (BAND_LO + BAND_HI)


def band_of(k):
    """Band of (real) bin index k >= 1: (bits of float32(k) >> 19) - 127 * 16, clamped (kernels.h: spec_band)."""
    k32 = np.atleast_1d(np.asarray(k, dtype=np.float32))
    return np.clip((k32.view(np.uint32) >> 19).astype(np.int64) - 127 * 16, 0, N_BANDS - 1)


def band_energy(x, P):
    """|FFT_P(x - mean)|^2 of the bins 1 .. P/2 - 1 summed into the detector's bands, float64 [384]."""
    xc = np.asarray(x, dtype=np.float64)
    xc = xc - xc.mean()
    return band_energy_of_spectrum(fft(xc, n=P), P)


def band_energy_of_spectrum(X, P):
    E = np.abs(X[1:P // 2]) ** 2
    band = (np.arange(1, P // 2, dtype=np.float32).view(np.uint32) >> 19).astype(np.int64) - 127 * 16
    return np.bincount(band, weights=E, minlength=N_BANDS)[:N_BANDS]


def _cover(a, b):
    """Fraction of every band inside [a, b)."""
    return np.clip(np.minimum(BAND_HI, b) - np.maximum(BAND_LO, a), 0.0, None) / (BAND_HI - BAND_LO)


def level_weights(lv, P, with_inexact=False):
    """w_b of one entry of ``debug_levels``; ``with_inexact``: also the bands whose weight float32 cannot hold exactly."""
    top = P / lv["decimation"]
    U = lv["band_shift"] * top / GRID
    w = _cover(0.0, top - U)
    if U > 0:
        w = w + _cover(0.0, U)
    inexact = w != np.round(w)                    # a band the level's top (or the shift) cuts through
    k1 = lv["low_cut"] * P / (2 * np.pi)
    k0 = 0.5 * k1
    if lv["low_cut"] > 0 and k1 - k0 >= 1:
        t = 0.5 - 0.5 * np.cos(np.pi * np.clip((BAND_MID - k0) / (k1 - k0), 0.0, 1.0))
        w = w * t * t
        # centres inside the transition, and those within float32 rounding of its ends
        inexact = inexact | ((BAND_MID >= k0 * (1 - 1e-6)) & (BAND_MID <= k1 * (1 + 1e-6)))
    return (w, inexact) if with_inexact else w


def plan_tables(plan, epoch=0):
    """What ``predict`` needs from a plan, gathered once: levels (the hook's low cut is the owner's), the level of
    every scale, kernel lengths, the gains on each scale's level grid."""
    levels = plan.debug_levels(epoch)
    level_of = level_of_scale(plan)
    length = plan.scale_info()["length"]
    gains = np.zeros((len(level_of), GRID))
    j = np.arange(GRID)
    for s, l in enumerate(level_of):
        if l >= 0:
            lv = levels[l]
            g = plan.debug_exact_gain(s, j - lv["band_shift"], GRID * lv["decimation"])
            gains[s] = g.astype(np.float32).astype(np.float64)
    return {"levels": levels, "level_of": level_of, "length": length, "gains": gains}


def predict(plan, h, P, kappa=KAPPA, oob=OOB, tables=None, damage=None):
    """{"rounding": [S], "left_out": [S], "level_energy": [n_levels], "predicted": [S], plus the sums "e_s", "e_out",
    "w_s" [S]} in float64.  ``damage``: one of 'one_minimum', 'own_cut', 'no_shift_in_density', 'bands_plus_one',
    'wrong_level' (module docstring); ``tables['own_cut']`` must hold each level's own cut for 'own_cut'."""
    tb = tables if tables is not None else plan_tables(plan)
    levels, level_of, gains = tb["levels"], tb["level_of"], tb["gains"]
    h = np.asarray(h, dtype=np.float64)
    if damage == "bands_plus_one":
        h = np.concatenate([[0.0], h[:-1]])
    S, nl = len(level_of), len(levels)
    e_level, outs, inexact = np.zeros(nl), [None] * nl, [None] * nl
    for l, lv in enumerate(levels):
        if damage == "own_cut":
            lv = dict(lv, low_cut=tb["own_cut"][l])
        w, inexact[l] = level_weights(lv, P, with_inexact=True)
        e_level[l] = (w * h).sum()
        outs[l] = (1.0 - np.minimum(w, 1.0)) * h
    res = {k: np.zeros(S) for k in ("rounding", "left_out", "e_s", "e_out", "w_s", "h_inexact")}
    j = np.arange(GRID)
    for s, l in enumerate(level_of):
        if l < 0:
            continue
        lv = levels[l]
        shift, top = lv["band_shift"], P / lv["decimation"]
        per_bin = top / GRID
        kc = np.abs((j - (0 if damage == "no_shift_in_density" else shift) + 0.5) * per_bin)
        b = band_of(np.maximum(kc, 1.0))
        dens = h[b] / np.maximum(1.0, BAND_HI[b] - BAND_LO[b]) * per_bin
        g2 = gains[s] ** 2
        side = np.zeros(GRID, dtype=np.int64) if damage == "one_minimum" else (j < shift).astype(np.int64)
        key = side * N_BANDS + b
        gmin = np.full(2 * N_BANDS, np.inf)
        np.minimum.at(gmin, key, g2)
        e_s = (gmin[key] * dens).sum()
        w_s = g2.sum() / GRID
        rise = np.ones(N_BANDS)
        if shift == 0:
            below = BAND_MID < top
            rise[below] = np.minimum(1.0, 2.0 * float(tb["length"][s]) * BAND_MID[below] / P)
        e_out = (rise * rise * outs[l]).sum()
        el = e_level[(l + 1) % nl if damage == "wrong_level" else l]
        res["e_s"][s], res["e_out"][s], res["w_s"][s] = e_s, e_out, w_s
        res["h_inexact"][s] = (rise * rise * h)[inexact[l]].sum()
        if e_s > 0:
            res["rounding"][s] = kappa * np.sqrt(el * w_s / e_s)
            res["left_out"][s] = oob * np.sqrt(e_out / e_s)
    res["level_energy"] = e_level
    res["level_h_inexact"] = np.array([h[i].sum() for i in inexact])
    res["predicted"] = np.maximum(res["rounding"], res["left_out"])
    res["sum_h"] = float(h.sum())
    return res


def tolerance(model, oob=OOB):
    """The bound on |kernel - model| for each term, from the model's own quantities: {"rounding", "left_out",
    "level_energy", "predicted", "abs_part", "rel_part", "left_out_loose"}.  rounding: REL_TOL relative.  left_out:
    REL_TOL on E_out plus the absolute error of 1 - w on it, through the root.  That error is at most ABS_WEIGHT per
    band, and none at all where float32 holds the weight exactly: w = 0 (band above the level's top, centre at or below
    k0: cover() and the taper return 0), w = 1 or 2 (band inside, centre at or above k1: x / (hi - lo) with x = hi - lo,
    t = 1).  So the absolute part is ABS_WEIGHT sum(r_b^2 h_b) over the bands a boundary cuts or whose centre lies in a
    cut's transition -- never more than ABS_WEIGHT sum(h), the cruder figure ("left_out_loose" is the bound with that
    one; the CPU tests hold this bound under it).  level_energy (a sum of w h): both parts, unrooted."""
    e_s, e_out = model["e_s"], model["e_out"]
    ok = e_s > 0
    safe = np.where(ok, e_s, 1.0)
    root = np.sqrt(e_out / safe)
    full = oob * (np.sqrt((e_out * (1 + REL_TOL) + ABS_WEIGHT * model["h_inexact"]) / safe) - root)
    loose = oob * (np.sqrt((e_out * (1 + REL_TOL) + ABS_WEIGHT * model["sum_h"]) / safe) - root)
    rel = oob * (np.sqrt(e_out * (1 + REL_TOL) / safe) - root)
    full, rel, loose = np.where(ok, full, 0.0), np.where(ok, rel, 0.0), np.where(ok, loose, 0.0)
    t_round = REL_TOL * model["rounding"]
    return {"rounding": t_round, "left_out": full, "predicted": np.maximum(t_round, full),
            "level_energy": REL_TOL * model["level_energy"] + ABS_WEIGHT * model["level_h_inexact"],
            "rel_part": rel, "abs_part": full - rel, "left_out_loose": loose}


# ---- cases ---------------------------------------------------------------------------------------------------------
# n_total of A2: the two epochs of the batch end at 116001; the third, shorter one (a smaller FFT: a batch of its own)
# lies behind them.
CASES = {
    "A": dict(n=1 << 17, f=(200.0, 0.5, 24), gamma=3.0, beta=20.0),
    "F34": dict(n=60000, f=(100.0, 1.5, 20), gamma=3.0, beta=4.0),
    "M4": dict(n=30000, f=(200.0, 5.0, 16), morlet_w0=4.0),
    "M6": dict(n=30000, f=(200.0, 5.0, 16), morlet_w0=6.0),
    "D": dict(n=30000, f=(480.0, 5.0, 20), gamma=3.0, beta=20.0),
    "A2": dict(n=146005, f=(200.0, 0.5, 24), gamma=3.0, beta=20.0,
               epochs=[[3, 58001], [58007, 116001], [116010, 146003]]),
}
RECORDINGS = ("pink", "line100", "drift1000", "white")
A2_CHANNELS = ("pink", "line100", "drift1000")


def frequencies(case):
    return np.geomspace(*CASES[case]["f"])


def make_plan(case, precision="high", n_channels=1, **kw):
    from ghost_amd.engine import CwtPlan
    c = CASES[case]
    args = {k: c[k] for k in ("gamma", "beta", "morlet_w0") if k in c}
    if "epochs" in c:
        args["epoch_bounds"] = c["epochs"]
    args.update(kw)
    return CwtPlan(c["n"], n_channels, FS, frequencies(case), precision=precision, **args)


def line(n, amp, freq=60.0, phase=0.3):
    """Pink LFP plus a line at ``amp`` times its spread, float32."""
    from ghost_amd.synthetic import lfp_channel
    base = lfp_channel(n, FS, 0).astype(np.float64)
    return (base + amp * base.std() * np.sin(2 * np.pi * freq * np.arange(n) / FS + phase)).astype(np.float32)


def recording(name, n):
    """float32 [n]: 'pink' (synthetic.lfp), 'line100' (60 Hz at 100 x its spread), 'drift1000' (0.05 Hz at 1000 x),
    'white'."""
    from ghost_amd.synthetic import lfp_channel
    if name == "pink":
        return lfp_channel(n, FS, 0)
    if name == "line100":
        return line(n, 100.0)
    if name == "drift1000":
        return line(n, 1000.0, 0.05, 0.0)
    if name == "white":
        return np.random.default_rng(4321).standard_normal(n).astype(np.float32)
    raise ValueError(name)


def segment_band_energy(x, start, stop, P):
    """Band energies of one segment as the engine sees it: the recording minus its GLOBAL mean, the segment's samples
    behind the lead that puts its start on a multiple of 64, zero-padded to P."""
    xc = np.asarray(x, dtype=np.float64)
    xc = xc - xc.mean()
    seg = np.concatenate([np.zeros(start & 63), xc[start:stop]])
    return band_energy_of_spectrum(fft(seg, n=P), P)


def a2_recording():
    """float32 [3][n]: pink, line100 and drift1000 on three channels."""
    return np.stack([recording(r, CASES["A2"]["n"]) for r in A2_CHANNELS])


def a2_model(plan, with_tolerance=False):
    """The model's prediction [segment][channel][scale] of A2 (and its bound), each segment on its own FFT."""
    x = a2_recording()
    segs = plan.segments()
    pred = np.zeros((len(segs), 3, plan.n_freqs))
    tol = np.zeros_like(pred)
    for e, (a, b, P) in enumerate(segs):
        tb = plan_tables(plan, epoch=e)
        for c in range(3):
            m = predict(plan, segment_band_energy(x[c], a, b, P), P, tables=tb)
            pred[e, c], tol[e, c] = m["predicted"], tolerance(m)["predicted"]
    return (pred, tol) if with_tolerance else pred
