"""Shared pieces of the Morlet tests (plain module, no fixtures): the float64 truth of a transform() row, the default
grid transform() builds, the layouts the CPU model and the device tests both use, and the level / kernel bookkeeping
of a Morlet plan (planning needs no GPU)."""
import numpy as np

from oracle import ghost_oracle as orc

TOL = 1e-5                      # the project's gate, per row against the row's peak (conftest.rel_err)
MODEL_TOL = 2.5e-6              # a quarter of it: what the float64 model of the fast path may use up
W0S = [2.0, 4.0, 5.0, 5.5, 6.0, 10.0, 20.0]
TWO_SIDED_BELOW = 5.6           # every w0 below has a two-sided band at the default band tolerance ("Morlet")
FOUR_EPOCHS = np.array([[0, 30011], [30011, 71011], [80000, 80700], [90000, 250000]])
FOUR_EPOCHS_N = 250000
FOUR_EPOCHS_F = np.geomspace(300.0, 1.0, 40)


def truth(x, fs, freqs, w0, rows=None, bounds=None, threads=1):
    """complex128 rows of one channel: per epoch, overlap_add_convolve(x - mean(x), psi_f, 'same'); 0 between.
    ``threads``: rows made side by side (the FFTs release the interpreter)."""
    from ghost_amd.wave import Morlet
    x64 = np.asarray(x, dtype=np.float64)
    xc = x64 - x64.mean()                                    # the global mean (transforms.py:142-143)
    rows = range(len(freqs)) if rows is None else rows
    bounds = [(0, x64.size)] if bounds is None else bounds
    out = np.zeros((len(rows), x64.size), dtype=np.complex128)

    def one(i):
        psi = Morlet(w0=w0, freq=freqs[rows[i]], fs=fs).get_wavelet()
        for a, b in bounds:
            out[i, a:b] = orc.overlap_add_convolve(xc[a:b], psi, mode="same")
    rows = list(rows)
    if threads > 1 and len(rows) > 1:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(threads) as pool:
            list(pool.map(one, range(len(rows))))
    else:
        for i in range(len(rows)):
            one(i)
    return out


def truth_window(x, mean, fs, freq, w0, a, b):
    """Columns [a, b) of the truth row of one whole-recording epoch, from a slice wide enough for the kernel."""
    from ghost_amd.wave import Morlet
    psi = Morlet(w0=w0, freq=freq, fs=fs).get_wavelet()
    lo, hi = max(0, a - len(psi)), min(len(x), b + len(psi))      # a cut end lies a whole kernel away from [a, b)
    assert hi - lo > len(psi)
    y = orc.overlap_add_convolve(np.asarray(x[lo:hi], dtype=np.float64) - mean, psi, mode="same")
    return y[a - lo:b - lo]


def as_output(output, c):
    return c if output == "complex" else np.abs(c) if output == "amplitude" else np.abs(c) ** 2


def gate(output):
    return 2 * TOL if output == "power" else TOL


def default_grid(w0, n, fs, voices=10):
    """transform()'s grid arithmetic (wave/transforms.py: freq_bounds_ref, n_octaves, j)."""
    from ghost_amd.wave import Morlet
    lo, hi = np.array(Morlet(w0=w0, fs=fs).compute_freq_bounds(n)) / np.pi * fs / 2.0
    j = np.arange(np.floor(np.log2(hi / lo) * voices) + 1)
    return hi / 2 ** (j / voices)


def levels(plan):
    """The plan's levels that hold scales, each with "scales": the rows on it.  A scale finds its level by
    (decimation, halo, hop): a Morlet plan can hold two levels of one decimation."""
    from ghost_amd import _lib
    si = plan.scale_info()
    lv = plan.debug_levels()
    keys = [(l["decimation"], l["halo"], l["hop"]) for l in lv]
    assert len(set(keys)) == len(keys), keys
    spectral = si["method"] == _lib.SCALE_SPECTRAL
    for l in lv:
        l["scales"] = np.flatnonzero(spectral & (si["decimation"] == l["decimation"]) & (si["halo"] == l["halo"]) &
                                     (si["hop"] == l["hop"]))
    assert sum(l["scales"].size for l in lv) == spectral.sum()
    return [l for l in lv if l["scales"].size]


def kernel(level, synth16=False):
    """The synthesis kernel of a Morlet plan's level (work_items.cpp: level_kernel; no interpolating synthesis):
    "k_synth", "k_synth7" or "k_synth7w" (the WIDE instantiation: halo > 48, shifted bands only)."""
    if level["band_shift"] == 0 and (synth16 or level["halo"] > 48 or level["scales"].size > 256):
        return "k_synth"
    assert level["scales"].size <= 256
    return "k_synth7w" if level["halo"] > 48 else "k_synth7"


def groups(plan):
    """{(method, decimation, halo): rows} over every scale of the plan."""
    si = plan.scale_info()
    out = {}
    for i, key in enumerate(zip(si["method"].tolist(), si["decimation"].tolist(), si["halo"].tolist())):
        out.setdefault(key, []).append(i)
    return out


def row_subset(plan, rng, whole=(), extra=4):
    """A seeded subset of rows: every row of the groups `whole` names (a predicate on (method, decimation, halo)), one
    of every other group, and `extra` more."""
    g = groups(plan)
    rows = set(rng.choice(plan.n_freqs, extra).tolist())
    for key, v in g.items():
        rows |= set(v) if whole and whole(key) else {int(rng.choice(v))}
    rows = sorted(rows)
    si = plan.scale_info()
    assert {(si["method"][r], si["decimation"][r], si["halo"][r]) for r in rows} == set(g)
    return rows
