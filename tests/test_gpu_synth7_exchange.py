"""k_synth7's scale loop where the exchange between its two DFT16 passes stays inside a wavefront (R <= 4: no
workgroup barrier around it, kernels.h: synth7_exchange_wave_local) next to where it does not (R = 8: both barriers).

The smallest layout at which each path and its neighbour run: 2 channels x 30 000 samples at 1 kHz, twelve scales from
200 Hz down to 40 Hz -- levels R = 2, 4 and 8, all on k_synth7 (asserted through scale_info() / debug_levels()).  With
hop 212 .. 216 a workgroup covers 1 700 (16 columns, R = 2) to 6 900 samples (32 columns, R = 4): every level has a
first, interior and last group of blocks.  The option synth7_narrow_r sends R = 2 to the 32-column instantiation (0),
R = 2 to the 16-column one (2, the default) and R = 4 there as well (4), so both instantiations run wave-local at both
decimations.

Checked: the whole transform against the float64 oracle on the project's metric (max |y - ref| / max |ref| per row) at
its 1e-5 gate, amplitude, power and complex; block requests whose windows start and end inside a group of blocks at
odd offsets, bit-equal to the same columns of the whole transform (workgroups cut by the window next to whole ones); a
two-epoch plan (two segments on one grid, workgroups of the shorter one leave early); Morse pairs whose bands are
shifted below zero (deep and wide halos among them) and Morlet plans (the complex-gain instantiation) at R <= 4; and
that an execute repeated gives the same bits (waves no longer wait for each other inside a chunk of scales)."""
import numpy as np
import pytest

from conftest import rel_err
from morlet_cases import levels as _plan_levels, truth as _morlet_truth
from oracle import ghost_oracle as orc

pytestmark = pytest.mark.gpu

TOL = 1e-5
FS, N = 1000.0, 30000
F12 = np.geomspace(200.0, 40.0, 12)
OUTPUTS = ["amplitude", "power", "complex"]
TWO_EPOCHS = np.array([[0, 9001], [10003, 24000]])     # both on FFTs of 2^14: one batch, one grid
# windows that start and end inside a group of blocks, at odd offsets: across most of the recording, one group wide,
# inside one block, one sample, the recording's two ends
WINDOWS = [(1, 29998), (3391, 6785), (6989, 13001), (12345, 1), (20211, 431), (0, 1001), (28999, 1001)]
_CACHE = {}


def _x():
    if "x" not in _CACHE:
        from ghost_amd.synthetic import lfp
        _CACHE["x"] = np.ascontiguousarray(lfp(2, N, FS, seed=212), dtype=np.float32)
    return _CACHE["x"]


def _morse_ref(f, bounds=None, gamma=3.0, beta=20.0):
    """complex128 (2, len(f), N), made once per layout and never written to."""
    key = ("morse", tuple(np.asarray(f).tolist()), None if bounds is None else tuple(map(tuple, bounds)), gamma, beta)
    if key not in _CACHE:
        x = _x()
        ref = np.stack([orc.cwt_complex(x[c].astype(np.float64), FS, np.asarray(f), bounds, gamma=gamma, beta=beta)
                        for c in range(x.shape[0])])
        ref.setflags(write=False)
        _CACHE[key] = ref
    return _CACHE[key]


def _morlet_ref(f, w0):
    key = ("morlet", tuple(np.asarray(f).tolist()), w0)
    if key not in _CACHE:
        x = _x()
        ref = np.stack([_morlet_truth(x[c], FS, np.asarray(f), w0) for c in range(x.shape[0])])
        ref.setflags(write=False)
        _CACHE[key] = ref
    return _CACHE[key]


def _as(output, c):
    return c if output == "complex" else np.abs(c) if output == "amplitude" else np.abs(c) ** 2


def _levels(plan, want_r, max_halo=48):
    """The plan's levels: nothing interpolated, every level on k_synth7 (at most 256 scales; halo <= 48 or a shifted
    band), the decimations `want_r` among them with halo <= max_halo.  Returns {decimation: [levels]}."""
    from ghost_amd import _lib
    assert plan.info["n_interp"] == 0
    lv = _plan_levels(plan)
    si = plan.scale_info()
    assert lv and np.all(si["method"][np.concatenate([l["scales"] for l in lv])] == _lib.SCALE_SPECTRAL)
    by = {}
    for l in lv:
        assert l["scales"].size <= 256 and (l["halo"] <= 48 or l["band_shift"] > 0), l
        by.setdefault(l["decimation"], []).append(l)
    for r in want_r:
        assert any(l["halo"] <= max_halo for l in by.get(r, [])), (r, lv)
    return by


def _spectral_rows(plan):
    return np.sort(np.concatenate([l["scales"] for l in _plan_levels(plan)]))


def _gate(name, got, ref, output, rows=None):
    rows = slice(None) if rows is None else rows
    err = np.stack([rel_err(got[c][rows], _as(output, ref[c][rows])) for c in range(got.shape[0])])
    print("%s %s: worst row %.3g (gate %.0e), median %.3g" % (name, output, err.max(), TOL, np.median(err)))
    assert err.max() < TOL, (name, output, err.max(), np.unravel_index(np.argmax(err), err.shape))


@pytest.mark.parametrize("narrow_r", [0, 2, 4])
@pytest.mark.parametrize("output", OUTPUTS)
def test_whole_transform_meets_the_oracle(option, output, narrow_r):
    from ghost_amd.engine import CwtPlan
    option("synth7_narrow_r", narrow_r)
    plan = CwtPlan(N, 2, FS, F12, output=output)
    by = _levels(plan, (2, 4, 8))
    assert all(l["band_shift"] == 0 and 16 <= l["halo"] <= 32 for ls in by.values() for l in ls)
    # first, interior and last groups of blocks at every level: more than two groups of 32 (16) columns
    for r, ls in by.items():
        cols = 16 if r <= narrow_r else 32
        assert all(l["nblk"] > 2 * max(1, cols // r) for l in ls), (r, ls)
    got = plan.execute(_x())
    _gate("whole, narrow_r=%d" % narrow_r, got, _morse_ref(F12), output)
    np.testing.assert_array_equal(plan.execute(_x()), got)
    plan.close()


@pytest.mark.parametrize("narrow_r", [0, 2, 4])
@pytest.mark.parametrize("output", OUTPUTS)
def test_block_requests_are_the_whole_transforms_columns(option, output, narrow_r):
    from ghost_amd.engine import CwtPlan
    option("synth7_narrow_r", narrow_r)
    plan = CwtPlan(N, 2, FS, F12, output=output)
    _levels(plan, (2, 4, 8))
    x = _x()
    whole = plan.execute(x)
    for start, length in WINDOWS:
        assert start % 2 == 1 or (start + length) % 2 == 1
        blk = plan.execute_block(x, start, length)
        np.testing.assert_array_equal(blk, whole[..., start:start + length], err_msg="%d + %d" % (start, length))
    plan.close()


@pytest.mark.parametrize("output", OUTPUTS)
def test_two_epochs_share_a_grid(output):
    from ghost_amd.engine import CwtPlan
    plan = CwtPlan(N, 2, FS, F12, epoch_bounds=TWO_EPOCHS, output=output)
    _levels(plan, (2, 4, 8))
    assert plan.debug_batches() == [(0, 2)]
    x = _x()
    got = plan.execute(x)
    _gate("two epochs", got, _morse_ref(F12, TWO_EPOCHS), output)
    gap = slice(int(TWO_EPOCHS[0, 1]), int(TWO_EPOCHS[1, 0]))
    assert not np.any(got[..., gap])
    assert not np.any(got[..., int(TWO_EPOCHS[1, 1]):])
    for start, length in [(8001, 4003), (1, 9000), (10003, 1), (15555, 14445)]:   # across the gap; inside an epoch; past the end
        np.testing.assert_array_equal(plan.execute_block(x, start, length), got[..., start:start + length],
                                      err_msg="%d + %d" % (start, length))
    plan.close()


SHIFTED = {
    # Morse(3, 6): shifted bands at R = 2, 4, 8, halo 24 .. 26
    "beta6": dict(f=np.geomspace(120.0, 20.0, 10), gamma=3.0, beta=6.0, max_halo=32),
    # Morse(3, 4): R = 2 with halo 46 (rows 2 / 13 lane-wise) and 66 (the wide-halo instantiation), R = 4 with halo 41
    "beta4": dict(f=np.geomspace(120.0, 20.0, 10), gamma=3.0, beta=4.0, max_halo=48),
}


@pytest.mark.parametrize("output", ["amplitude", "complex"])
@pytest.mark.parametrize("pair", sorted(SHIFTED))
def test_shifted_bands(pair, output):
    from ghost_amd.engine import CwtPlan
    s = SHIFTED[pair]
    plan = CwtPlan(N, 2, FS, s["f"], gamma=s["gamma"], beta=s["beta"], output=output)
    by = _levels(plan, (2, 4), max_halo=s["max_halo"])
    assert all(l["band_shift"] > 0 for ls in by.values() for l in ls), by
    if pair == "beta4":
        assert any(l["halo"] > 48 for l in by[2]) and any(32 < l["halo"] <= 48 for l in by[2] + by[4]), by
    x = _x()
    got = plan.execute(x)
    _gate("Morse(%g, %g)" % (s["gamma"], s["beta"]), got, _morse_ref(s["f"], gamma=s["gamma"], beta=s["beta"]), output,
          rows=_spectral_rows(plan))
    np.testing.assert_array_equal(plan.execute_block(x, 3391, 6785), got[..., 3391:3391 + 6785])
    plan.close()


@pytest.mark.parametrize("output", ["amplitude", "complex"])
@pytest.mark.parametrize("w0", [6.0, 4.0])
def test_morlet_plans(w0, output):
    """The complex-gain instantiation: w0 = 6 on unshifted bands (R = 2, 4), w0 = 4 on shifted ones (halo 32 / 33)."""
    from ghost_amd.engine import CwtPlan
    plan = CwtPlan(N, 2, FS, F12, morlet_w0=w0, output=output)
    by = _levels(plan, (2, 4))
    assert all((l["band_shift"] > 0) == (w0 == 4.0) for ls in by.values() for l in ls), by
    x = _x()
    got = plan.execute(x)
    _gate("Morlet(%g)" % w0, got, _morlet_ref(F12, w0), output, rows=_spectral_rows(plan))
    np.testing.assert_array_equal(plan.execute_block(x, 3391, 6785), got[..., 3391:3391 + 6785])
    plan.close()
